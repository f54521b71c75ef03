"""Lesion-wise Dice and HD95 of a written prediction against its ground truth, on the device (L1-L3,
csrc/gts_lesionwise.hip; definition and deviations from the BraTS 2023 script: DESIGN.md 4o).

Per region (WT, CT, ET): the truth mask G is dilated (L1), the 26-connected components of the dilated mask D
are the lesions and those of the predicted mask P the predicted components (C1-C3); one pass (L2) gives each
lesion's volume, true positives and box, each component's size and box, and the (component, lesion) pairs that
touch.  The tables come to the host in one copy; per scored lesion the masks M_k and G_k are written over the
lesion's box (L3) and go through the HD95 kernels (H1-H5).  The float arithmetic is one division per lesion,
gts.metrics.percentile95_from_order_stats, and sequential float64 sums in lesion order.  With a voxel spacing the
per-lesion pair goes through the weighted kernels instead (H3w-H5w): HD95 in millimetres and, with
tolerances, the normalised surface Dice per lesion from the same call.

Labels are internal: 0 healthy, 1 edema, 2 NET, 3 ET.  Everything runs on the current stream.
"""
import ctypes

import numpy as np
import torch

from . import _lib, _volume, components, metrics
from ._lesions import REGIONS, region_index, region_mask, table_head
from ._lib import check, current_stream, ptr

DILATIONS = (0, 1, 2, 3)
PENALTY_HD95 = 374.0         # HD95 of a missed lesion and of a false-positive component
ROW_INTS = 9                 # root | count | tp | box (gts_lesionwise_tables_i16)


def _dilation(dilation, what):
    if isinstance(dilation, bool) or dilation not in DILATIONS:
        raise _lib.GtsError(f"{what}: dilation {dilation!r} (one of {DILATIONS})")
    return int(dilation)


def dilate_region(labels, region, dilation=3):
    """int16 0 / 1 tensor of labels' shape: scipy's binary_dilation(region mask of labels,
    generate_binary_structure(3, 2), iterations=dilation), clipped at the volume.  labels: int16 CUDA tensor
    [X, Y, Z] of internal labels; region "WT", "CT" or "ET" (or 0..2); dilation 0..3."""
    labels = _volume.label_volume(labels, "dilate_region", three_d=True)
    region, dilation = region_index(region, "dilate_region"), _dilation(dilation, "dilate_region")
    lib = _lib.load()
    workspace, size = _volume.workspace(lib.gts_lesionwise_workspace, *labels.shape, labels.device, "dilate_region")
    return region_mask(lib, labels, region, dilation, workspace, size)


def _box(row, shape):
    """(begin, end) per axis of a table row's box."""
    return [(shape[a] - int(row[4 + 2 * a]), int(row[3 + 2 * a])) for a in range(3)]


class _RegionState:
    """What one region's device pass leaves for the per-lesion masks."""

    def __init__(self, lib, pred, truth, region, dilation):
        what = "lesion_tables"
        self.lib, self.truth, self.region, self.shape = lib, truth, region, tuple(truth.shape)
        x, y, z = self.shape
        workspace, size = _volume.workspace(lib.gts_lesionwise_workspace, x, y, z, truth.device, what)
        mask_p, mask_d = (region_mask(lib, v, region, n, workspace, size) for v, n in ((pred, 0), (truth, dilation)))
        self.roots_p = components.roots_unchecked(mask_p, self.shape, 26, what)
        self.roots_d = components.roots_unchecked(mask_d, self.shape, 26, what)
        ints = lib.gts_lesionwise_table_ints(x, y, z)
        block = torch.empty(ints, dtype=torch.int32, device=truth.device)
        check(lib.gts_lesionwise_tables_i16(ptr(truth), ptr(self.roots_p), ptr(self.roots_d), x, y, z, region,
                                            ptr(block), ints, ptr(workspace), size, current_stream()),
              "gts_lesionwise_tables_i16")
        head = table_head(block, lambda head: 4 + ROW_INTS * (int(head[0]) + int(head[1])) + 2 * int(head[2]))
        n_l, n_c, n_p = (int(v) for v in head[:3])
        rows = head[4:4 + ROW_INTS * (n_l + n_c)].reshape(n_l + n_c, ROW_INTS).astype(np.int64)
        lesions, comps = rows[:n_l], rows[n_l:]
        self.lesions = lesions[np.argsort(lesions[:, 0])]          # scipy's label order: by smallest index
        self.comps = comps[np.argsort(comps[:, 0])]
        pairs = head[4 + ROW_INTS * (n_l + n_c):].reshape(n_p, 2).astype(np.int64)
        self.pairs = np.unique(pairs, axis=0) if n_p else pairs      # (component root, lesion root), sorted
        self.matched_dev = None

    def tables(self):
        lesion_of = {int(r): k for k, r in enumerate(self.lesions[:, 0])}
        comp_of = {int(r): c for c, r in enumerate(self.comps[:, 0])}
        matched = [[] for _ in lesion_of]
        hit = np.zeros(len(comp_of), dtype=bool)
        for comp_root, lesion_root in self.pairs.tolist():
            matched[lesion_of[lesion_root]].append(comp_of[comp_root])          # ascending component order
            hit[comp_of[comp_root]] = True
        sizes = self.comps[:, 1]
        return dict(lesion_roots=self.lesions[:, 0].tolist(), vol=self.lesions[:, 1].tolist(),
                    tp=self.lesions[:, 2].tolist(),
                    matched_voxels=[int(sizes[m].sum()) if m else 0 for m in matched],
                    matched_components=matched, comp_roots=self.comps[:, 0].tolist(), comp_sizes=sizes.tolist(),
                    n_fp=int((~hit).sum()))

    def lesion_masks(self, k, matched):
        """(M_k, G_k) over the union box of both, grown by one voxel and clamped: a mask voxel then lies on a
        face of the crop only where that is a face of the volume, so the crop's borders are the volume's."""
        lib = self.lib
        boxes = [_box(self.lesions[k], self.shape)] + [_box(self.comps[c], self.shape) for c in matched]
        crop = []
        for a in range(3):
            crop += [max(min(b[a][0] for b in boxes) - 1, 0), min(max(b[a][1] for b in boxes) + 1, self.shape[a])]
        if self.matched_dev is None:            # every lesion's matched roots, one upload per region
            order = np.argsort(self.pairs[:, 1], kind="stable")
            self.by_lesion = self.pairs[order]
            self.matched_dev = torch.from_numpy(self.by_lesion[:, 0].astype(np.int32)).to(self.truth.device)
        root = int(self.lesions[k, 0])
        first = int(np.searchsorted(self.by_lesion[:, 1], root, "left"))
        count = int(np.searchsorted(self.by_lesion[:, 1], root, "right")) - first
        dims = tuple(crop[2 * a + 1] - crop[2 * a] for a in range(3))
        mask_m = torch.empty(dims, dtype=torch.int16, device=self.truth.device)
        mask_g = torch.empty_like(mask_m)
        x, y, z = self.shape
        check(lib.gts_lesionwise_masks_i16(ptr(self.truth), ptr(self.roots_p), ptr(self.roots_d), x, y, z, self.region,
                                           root, self.matched_dev.data_ptr() + 4 * first, count,
                                           (ctypes.c_int64 * 6)(*crop), ptr(mask_m), ptr(mask_g), current_stream()),
              "gts_lesionwise_masks_i16")
        return mask_m, mask_g

    def lesion_hd95(self, k, matched):
        """hd95(M_k, G_k) in voxels."""
        n, d2_lo, d2_hi, present = metrics.hd95_order_stats(*self.lesion_masks(k, matched))[2].cpu().tolist()
        if present != 3:
            raise _lib.GtsError(f"lesionwise: lesion {k} lost a mask")
        return metrics.percentile95_from_order_stats(n, d2_lo, d2_hi)

    def lesion_surface(self, k, matched, spacing_mm, tolerances_mm):
        """(hd95 in mm, [NSD per tolerance]) of M_k against G_k, from one weighted call."""
        row = metrics.surface_stats(*self.lesion_masks(k, matched), spacing_mm, tolerances_mm)[2].cpu().tolist()
        if row[3] != 3:
            raise _lib.GtsError(f"lesionwise: lesion {k} lost a mask")
        return (metrics.hd95_mm_from_row(row, metrics.spacing_units(spacing_mm)[1]),
                metrics.surface_dices_from_row(row, len(tolerances_mm)))


def lesion_tables(pred, truth, region, dilation=3):
    """The integer tables of one region, as Python lists in lesion order (ascending smallest C-order index of
    the dilated lesion, scipy's label order): lesion_roots, vol (|G_k|), tp (|P n G_k|), matched_voxels (|M_k|),
    matched_components (indices into comp_roots / comp_sizes, which are in component order), n_fp."""
    pred, truth = _volume.label_pair(pred, truth, "lesion_tables", three_d=True)
    region, dilation = region_index(region, "lesion_tables"), _dilation(dilation, "lesion_tables")
    return _RegionState(_lib.load(), pred, truth, region, dilation).tables()


def _region_scores(state, min_lesion_voxels, spacing_mm=None, nsd_tolerances_mm=()):
    t = state.tables()
    n_tol = len(nsd_tolerances_mm)
    lesions, dice_sum, hd_sum, nsd_sum, n_scored, n_fn = [], 0.0, 0.0, [0.0] * n_tol, 0, 0
    for k, (vol, tp, m, matched) in enumerate(zip(t["vol"], t["tp"], t["matched_voxels"], t["matched_components"])):
        scored = vol > min_lesion_voxels
        dice = hd = nsd = None
        if scored:
            if m == 0:
                dice, hd, nsd = 0.0, PENALTY_HD95, [0.0] * n_tol
                n_fn += 1
            else:
                dice = (2 * tp) / (m + vol)
                if spacing_mm is None:
                    hd = state.lesion_hd95(k, matched)
                else:
                    hd, nsd = state.lesion_surface(k, matched, spacing_mm, nsd_tolerances_mm)
            dice_sum += dice
            hd_sum += hd
            nsd_sum = [a + b for a, b in zip(nsd_sum, nsd or ())]
            n_scored += 1
        lesion = dict(vol=vol, tp=tp, matched_voxels=m, scored=scored, dice=dice, hd95=hd)
        if n_tol:
            lesion["nsd"] = nsd
        lesions.append(lesion)
    n_fp = t["n_fp"]
    if n_scored + n_fp == 0:
        lw_dice, lw_hd95, lw_nsd = 1.0, 0.0, [1.0] * n_tol
    else:
        lw_dice = dice_sum / (n_scored + n_fp)
        lw_hd95 = (hd_sum + PENALTY_HD95 * n_fp) / (n_scored + n_fp)
        lw_nsd = [a / (n_scored + n_fp) for a in nsd_sum]
    record = dict(lw_dice=lw_dice, lw_hd95=lw_hd95, n_lesions=len(lesions), n_scored=n_scored, n_fp=n_fp, n_fn=n_fn,
                  lesions=lesions, lesion_roots=t["lesion_roots"])
    if n_tol:
        record["lw_nsd"] = lw_nsd
    return record


def lesionwise_scores(pred, truth, dilation=3, min_lesion_voxels=50, spacing_mm=None, nsd_tolerances_mm=()):
    """{"WT" | "CT" | "ET": record} for two int16 CUDA volumes [X, Y, Z] of internal labels.  A record holds
    the legacy whole-region dice (from the confusion counts) and hd95 (gts.metrics.hd95s), lw_dice, lw_hd95,
    n_lesions, n_scored, n_fp, n_fn and `lesions`: one dict per lesion in lesion order with vol, tp,
    matched_voxels, scored, dice and hd95 (None for a lesion of at most min_lesion_voxels voxels, which is
    not scored).  A scored lesion without a matched component has dice 0 and hd95 374, and so does every
    predicted component matched to no lesion.

    spacing_mm (x, y, z): the whole-region hd95 and every lesion's are in millimetres (gts.metrics.hd95s_mm);
    the penalty stays 374 and the dilation stays in voxels.  nsd_tolerances_mm (at most 4, needs a spacing):
    each record gains `nsd`, the whole-region surface Dice per tolerance (gts.metrics.surface_dices), and
    `lw_nsd`, its lesion-wise mean over lw_dice's divisor; each lesion gains `nsd` (None when not scored).  A
    missed lesion and a false-positive component count 0.  Without either the result is what it was."""
    from model import evaluation

    from . import ops

    pred, truth = _volume.label_pair(pred, truth, "lesionwise_scores", three_d=True)
    dilation = _dilation(dilation, "lesionwise_scores")
    nsd_tolerances_mm = tuple(nsd_tolerances_mm)
    if nsd_tolerances_mm and spacing_mm is None:
        raise _lib.GtsError("lesionwise_scores: nsd_tolerances_mm needs spacing_mm")
    lib = _lib.load()
    dices = evaluation.dices_from_confusion(ops.label_confusion(pred, truth).cpu().numpy())
    nsds = None
    if spacing_mm is None:
        hd95s = metrics.hd95s(pred, truth)
    else:
        spacing_mm = tuple(spacing_mm)
        scale = metrics.spacing_units(spacing_mm)[1]
        rows = metrics.surface_stats(pred, truth, spacing_mm, nsd_tolerances_mm).cpu().tolist()
        hd95s = [metrics.hd95_mm_from_row(row, scale) for row in rows]
        nsds = [metrics.surface_dices_from_row(row, len(nsd_tolerances_mm)) for row in rows]
    out = {}
    for r, name in enumerate(REGIONS):
        record = _region_scores(_RegionState(lib, pred, truth, r, dilation), min_lesion_voxels, spacing_mm,
                                nsd_tolerances_mm)
        record["dice"], record["hd95"] = float(dices[r]), float(hd95s[r])
        if nsd_tolerances_mm:
            record["nsd"] = nsds[r]
        out[name] = record
    return out
