"""Crop helpers used around the GNN path (counterpart of the functions of
/root/reference/data_processing/image_processing.py that the GNN scripts call)."""
import numpy as np
from scipy import ndimage

BRATS_SHAPE = (240, 240, 155)


def uncrop_to_brats_size(crop, voxel_preds):
    """Paste cropped predictions back into a zero (healthy) BraTS-sized int16 volume
    (reference image_processing.py:21-25)."""
    full = np.zeros(BRATS_SHAPE, dtype=np.int16)
    full[crop] = voxel_preds
    return full


def uncrop_maps_to_brats_size(crop, maps):
    """uncrop_to_brats_size for a stack of uint8 maps [K, x, y, z] (the uncertainty maps of gts.uncertainty):
    uint8 [K, *BRATS_SHAPE], zero (certain) outside the crop."""
    maps = np.asarray(maps)
    if maps.dtype != np.uint8 or maps.ndim != 4:
        raise ValueError(f"maps must be uint8 [K, x, y, z], got {maps.dtype} {maps.shape}")
    full = np.zeros((maps.shape[0],) + tuple(BRATS_SHAPE), dtype=np.uint8)
    for k in range(maps.shape[0]):
        full[k][crop] = maps[k]
    return full


def uncrop_to_shape(crop, voxel_preds, shape):
    """uncrop_to_brats_size for a volume of any shape: the cropped predictions pasted into a zero (healthy)
    int16 volume of `shape` (a scan conformed from another geometry has its own extents)."""
    full = np.zeros(tuple(int(n) for n in shape), dtype=np.int16)
    full[crop] = voxel_preds
    return full


def _any_along_other_axes(mask):
    return np.ix_(mask.any(axis=(1, 2)), mask.any(axis=(0, 2)), mask.any(axis=(0, 1)))


def determine_tumor_crop(preds):
    """Tightest box around the (dilated) predicted tumour; whole image when nothing is predicted
    (reference image_processing.py:8-17)."""
    mask = ndimage.binary_dilation(preds != 0)
    if not mask.any():
        print("No GNN predicted tumor, not cropping image")
        mask = ~mask
    return _any_along_other_axes(mask)


def tumor_crop_from_plane_flags(any_x, any_y, any_z):
    """determine_tumor_crop from the three per-axis `any` vectors of the UNdilated tumour mask
    (what K12's occupancy variant reports).  The 6-neighbourhood dilation of the reference adds,
    to the planes that hold tumour, exactly their two neighbours along the same axis, so the
    crop is the 1-D dilation of each vector; no tumour at all selects the whole volume."""
    flags = [np.asarray(v).astype(bool) for v in (any_x, any_y, any_z)]
    if not any(f.any() for f in flags):
        print("No GNN predicted tumor, not cropping image")
        return np.ix_(*[np.ones(len(f), dtype=bool) for f in flags])
    grown = []
    for f in flags:
        g = f.copy()
        g[1:] |= f[:-1]
        g[:-1] |= f[1:]
        grown.append(g)
    return np.ix_(*grown)


def determine_brain_crop(multi_modal_data):
    """Box of all planes that are not entirely black (reference image_processing.py:31-42)."""
    if multi_modal_data.ndim == 4:
        intensity = np.amax(multi_modal_data, axis=3)
    elif multi_modal_data.ndim == 3:
        intensity = multi_modal_data
    else:
        raise Exception(f"Expected input shape of either nxmxr or nxmxrxC. Instead got {multi_modal_data.shape}")
    return _any_along_other_axes(intensity > 0.01)



def normalize_img(img_array, is_flat=False):
    """Scale each channel by its 0.995 quantile taken as float32 (reference image_processing.py:45-51).
    Channels are the last axis; is_flat means [voxels, channels] instead of [X, Y, Z, channels]."""
    spatial_axes = 0 if is_flat else (0, 1, 2)
    top = np.quantile(img_array, 0.995, axis=spatial_axes).astype(np.float32)
    return img_array / top


def standardize_img(img_array, mean, std):
    """Per-channel z-score with given statistics (reference image_processing.py:53-56)."""
    return (img_array - mean) / std
