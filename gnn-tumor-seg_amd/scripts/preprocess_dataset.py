"""Raw BraTS scan folders -> supervoxel graph dataset (counterpart of the reference's
scripts/preprocess_dataset.py; same flags, defaults, standardization constants and outputs).

For each scan folder: the modalities are stacked, cropped to the planes that hold brain, the labels
moved to the internal coding, the intensities normalized and standardized, and the graph built by
mri2graph.graphgen.img2graph (SLIC, statistics and edges on the MI355X).  Written into
OUTPUT/{id}/: {id}_nxgraph.json, {id}_input.nii.gz, {id}_label.nii.gz (only with -l),
{id}_supervoxels.nii.gz and {id}_crop.npz (read back by data_loader.load_crop).

The GPU takes one scan at a time; decoding the next scans and encoding the finished ones run on a
small thread pool meanwhile.  A scan that raises is reported and left out; the exit status is 1
when any scan was left out.

    python -m scripts.preprocess_dataset -d RAW_DIR -l _seg.nii.gz -o OUT_DIR

Standardization uses the reference's BraTS-2021 constants unless --stats is given: --stats STATS.json takes
the values of a file written by scripts.compute_dataset_stats; --stats compute takes them first over the
input folder (needs -l), as the reference does when its constant is None, and writes
OUT_DIR/standardization.json.

--bias_correct (with --bias_levels, --bias_spans, --bias_iterations, --bias_tol, --bias_threshold, --bias_report, as
scripts.segment_scans documents them) removes each modality's bias field on the device (gts.bias)
before the crop, the normalization and, with --stats compute, the statistics: the graphs a model is trained on then
see the correction that `segment_scans --bias_correct` applies to the scans it segments.

--skull_strip [MODALITY] (with --strip_radius, --strip_close, --strip_fraction, --strip_connectivity, --strip_report, as
scripts.segment_scans documents them) sets every modality to 0 outside a brain mask found on the device (gts.brainmask,
DESIGN.md 4x) before all of that, --bias_correct included, for scans that still hold their skull.
"""
import argparse
import glob
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _PKG not in sys.path:
    sys.path.insert(0, _PKG)

import Filepaths  # noqa: E402
from data_processing import graph_io, nifti_io, standardization  # noqa: E402
from data_processing.data_loader import save_crop  # noqa: E402
from data_processing.image_processing import determine_brain_crop, normalize_img, standardize_img  # noqa: E402
from data_processing.labels import LABEL_MAP, swap_labels_from_brats  # noqa: E402,F401

# per-modality (mean, standard deviation) after normalization: the reference's fixed values
STANDARDIZATION_STATS = ([0.4645, 0.6625, 0.4064, 0.3648], [0.1593, 0.1703, 0.1216, 0.1627])
BRATS_MODALITIES = ["_flair.nii.gz", "_t1.nii.gz", "_t1ce.nii.gz", "_t2.nii.gz"]
IO_WORKERS = 3     # threads for NIfTI decode / encode around the GPU work
READ_AHEAD = 2     # scans decoded ahead of the one on the GPU

_FLAGS = (
    # short, long, default, type, help
    ("-d", "--data_dir", None, str, "folder holding the raw scan folders (default: Filepaths.INPUT_MRI_DIR)"),
    ("-n", "--num_nodes", 15000, int, "approximate number of SLIC supervoxels per scan"),
    ("-k", "--num_neighbors", 10, int, "edges per node of the kNN graph; 0 links supervoxels that touch instead"),
    ("-b", "--boxiness", 0.5, float, "SLIC compactness: larger gives more cube-like supervoxels"),
    ("-o", "--output_dir", None, str, "where the graph dataset goes (default: PROCESSED_DATA_DIR_n_b_k)"),
)


def build_parser():
    """Same flags and defaults as the reference CLI (scripts/preprocess_dataset.py:177-184)."""
    parser = argparse.ArgumentParser(description="Build supervoxel graphs from BraTS MRI folders on MI355X")
    for short, long_name, default, kind, text in _FLAGS:
        parser.add_argument(short, long_name, default=default, type=kind, help=text)
    parser.add_argument("-m", "--modality_extensions", nargs="+", default=list(BRATS_MODALITIES),
                        help="file suffix of each modality, in channel order")
    parser.add_argument("-l", "--label_extension", default=None,
                        help="file suffix of the label volume; without it no labels are read or written")
    parser.add_argument("-p", "--data_prefix", default="", help="common prefix of the scan folders, e.g. BraTS2021")
    parser.add_argument("--stats", default=None, metavar="STATS.json|compute",
                        help="standardization statistics: a file of scripts.compute_dataset_stats, or 'compute' to take "
                             "them over the input folder first (default: the BraTS-2021 constants)")
    from gts import bias, brainmask

    return brainmask.add_flags(bias.add_flags(parser))


def default_output_dir(args):
    return f"{Filepaths.PROCESSED_DATA_DIR}_{args.num_nodes}_{args.boxiness}_{args.num_neighbors}"


def find_scans(data_dir, prefix):
    """{scan id: folder} for every folder under data_dir whose name starts with prefix."""
    root = os.path.join(os.path.expanduser(data_dir), "")
    folders = glob.glob(f"{root}**/{prefix}*/", recursive=True)
    return {os.path.basename(os.path.normpath(f)): f for f in folders}


class DataPreprocessor:
    """Runs the per-scan pipeline over every scan folder of args.data_dir."""

    def __init__(self, args):
        self.args = args
        self.k = args.num_neighbors or None
        self.output_dir = os.path.expanduser(args.output_dir or default_output_dir(args))
        self.scans = find_scans(args.data_dir or Filepaths.INPUT_MRI_DIR, args.data_prefix)
        self.all_ids = sorted(self.scans)
        self.stats_failed = []
        from gts import bias, brainmask

        self.bias = bias.settings_from_args(args)       # None without --bias_correct
        self.bias_report = {}
        self.strip = brainmask.settings_from_args(args)  # None without --skull_strip
        self.strip_report = {}
        self.mean, self.std = self.standardization_stats(getattr(args, "stats", None))
        print(f"{len(self.all_ids)} scan folders found; graphs go to {self.output_dir}")

    def standardization_stats(self, stats):
        """(mean, std) float32: the constants, a statistics file's values, or ('compute') the input folder's own."""
        if not stats:
            return tuple(np.array(s, dtype=np.float32) for s in STANDARDIZATION_STATS)
        if stats != "compute":
            return standardization.load_stats(os.path.expanduser(stats), self.args.modality_extensions)
        from scripts import compute_dataset_stats

        path = os.path.join(self.output_dir, standardization.FILE_NAME)
        mean, std, self.stats_failed = compute_dataset_stats.compute_and_save(
            self.scans, self.args.modality_extensions, self.args.label_extension, path, bias_settings=self.bias,
            strip_settings=self.strip)
        print(f"standardization statistics over {len(self.scans) - len(self.stats_failed)} scan(s) written to {path}")
        return standardization.load_stats(path, self.args.modality_extensions)

    def load(self, scan_id):
        """Host stage: decode, crop, relabel, normalize, standardize."""
        folder = self.scans[scan_id]
        image = nifti_io.read_in_patient_sample(folder, self.args.modality_extensions)
        if self.bias is not None or self.strip is not None:     # stripped / corrected on the device first: run() calls
            # finish() for the rest of this stage
            labels = nifti_io.read_in_labels(folder, self.args.label_extension) if self.args.label_extension else None
            return image, labels, None
        crop = determine_brain_crop(image)
        labels = None
        if self.args.label_extension:
            labels = swap_labels_from_brats(nifti_io.read_in_labels(folder, self.args.label_extension)[crop])
        image = standardize_img(normalize_img(image[crop]), self.mean, self.std)
        return image, labels, crop

    def finish(self, scan_id, image, labels):
        """With --skull_strip or --bias_correct: the strip, then the correction, on the device, then what load() does to
        a scan taken as stored."""
        from gts import bias, brainmask

        if self.strip is not None:
            image, _, self.strip_report[scan_id] = brainmask.strip_image(image, self.strip[0], **self.strip[1])
        if self.bias is not None:
            image, self.bias_report[scan_id] = bias.correct_image(image, **self.bias)
        crop = determine_brain_crop(image)
        if labels is not None:
            labels = swap_labels_from_brats(labels[crop])
        return standardize_img(normalize_img(image[crop]), self.mean, self.std), labels, crop

    def store(self, scan_id, graph, image, labels, partition, crop):
        """Host stage: JSON + gzip NIfTI encode."""
        stem = os.path.join(self.output_dir, scan_id, scan_id)
        os.makedirs(os.path.dirname(stem), exist_ok=True)
        graph_io.save_networkx_graph(graph, stem + "_nxgraph.json")
        outputs = {"_input.nii.gz": image, "_label.nii.gz": labels, "_supervoxels.nii.gz": partition}
        for suffix, volume in outputs.items():
            if volume is not None:
                nifti_io.save_as_nifti(volume, stem + suffix)
        save_crop(stem + "_crop.npz", crop)

    def run(self):
        """Process every scan; returns the ids that failed."""
        from gts import bias, brainmask
        from mri2graph.graphgen import img2graph

        failed, writes = [], []
        ids = self.all_ids
        with ThreadPoolExecutor(max_workers=IO_WORKERS) as pool:
            pending = {i: pool.submit(self.load, ids[i]) for i in range(min(READ_AHEAD, len(ids)))}
            for i, scan_id in enumerate(ids):
                if i + READ_AHEAD < len(ids):
                    pending[i + READ_AHEAD] = pool.submit(self.load, ids[i + READ_AHEAD])
                try:
                    image, labels, crop = pending.pop(i).result()
                    if crop is None:
                        image, labels, crop = self.finish(scan_id, image, labels)
                    graph, _, partition = img2graph(image, labels, self.args.num_nodes, self.args.boxiness, self.k)
                except Exception as exc:
                    print(f"{scan_id}: skipped ({exc!r})")
                    failed.append(scan_id)
                    continue
                writes.append((scan_id, pool.submit(self.store, scan_id, graph, image, labels, partition, crop)))
            for scan_id, job in writes:
                try:
                    job.result()
                    note = f" ({brainmask.describe(self.strip_report[scan_id])})" if scan_id in self.strip_report else ""
                    note += f" ({bias.describe(self.bias_report[scan_id])})" if scan_id in self.bias_report else ""
                    print(f"{scan_id}: done{note}")
                except Exception as exc:
                    print(f"{scan_id}: writing failed ({exc!r})")
                    failed.append(scan_id)
        if getattr(self.args, "bias_report", None):
            bias.save_report(self.args.bias_report, self.args.modality_extensions, self.bias, self.bias_report)
        if getattr(self.args, "strip_report", None):
            brainmask.save_report(self.args.strip_report, self.args.modality_extensions, self.strip[0], self.strip[1],
                                  self.strip_report)
        return failed


def main(argv=None):
    args = build_parser().parse_args(argv)
    try:
        gen = DataPreprocessor(args)
    except ValueError as exc:                   # --bias_* or --strip_* settings that cannot run
        print(f"preprocess_dataset: {exc}", file=sys.stderr)
        return 2
    except standardization.StatsError as exc:   # a statistics file that does not fit this run, or none could be computed
        print(f"preprocess_dataset: {exc}", file=sys.stderr)
        return 2
    failed = gen.run()
    print(f"preprocessing finished, {len(failed)} scan(s) skipped")
    return 1 if failed or gen.stats_failed else 0


if __name__ == "__main__":
    sys.exit(main())
