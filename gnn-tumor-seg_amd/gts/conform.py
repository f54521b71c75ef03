"""Conform a scan of any orientation and voxel spacing to the frame the pipeline was built for, and carry
label volumes back (F1, csrc/gts_conform.hip).

The pipeline's frame is BRATS_AFFINE's: array axes run towards Left, Posterior, Superior ("LPS") at 1 mm.
plan(affine, shape) is pure numpy and runs without a GPU: the axis permutation, the flips, the spacings and the
per-axis index tables the kernel gathers by.  conform_scan / conform_labels / unconform_labels run the
kernel on device volumes laid out [C, Z, Y, X] or [Z, Y, X], x fastest, as intake.stage_scan lays them out.

A rotation left over after the closest axis assignment is dropped (as nibabel's closest-canonical does) and
reported as obliquity_deg; nothing is refused for being oblique.
"""
import itertools
from dataclasses import dataclass

import numpy as np

TARGET_SIGNS = (-1.0, -1.0, 1.0)       # array axes of the pipeline's frame run towards L, P, S (BRATS_AFFINE)
UNIT_SNAP = 1e-4                       # |s - 1| <= this: the spacing is taken as exactly 1
AFFINE_AGREEMENT = 1e-3                # modalities of one scan: largest absolute difference between affines
MODE_EXACT, MODE_TRILINEAR, MODE_NEAREST = 0, 1, 2
_LETTERS = (("L", "R"), ("P", "A"), ("I", "S"))


@dataclass(frozen=True)
class AxisTables:
    """How one output axis reads an input axis: idx0 / idx1 int32 [n_out], t float64 [n_out]."""
    idx0: np.ndarray
    idx1: np.ndarray
    t: np.ndarray

    @property
    def n_out(self):
        return len(self.idx0)


def forward_tables(n, s, reverse):
    """Tables of a conformed axis read from an input axis of length n at spacing s (mm), 1 mm out.
    n_out = floor((n - 1) s) + 1, so no sample falls outside the input; for output index i: u = i / s,
    r0 = min(floor(u), n - 1), r1 = min(r0 + 1, n - 1), t = u - r0; r0 and r1 go through the flip."""
    n, s = int(n), float(s)
    n_out = int(np.floor((n - 1) * s)) + 1
    u = np.arange(n_out, dtype=np.float64) / s
    r0 = np.minimum(np.floor(u), n - 1)
    r1 = np.minimum(r0 + 1, n - 1)
    t = u - r0
    if reverse:
        r0, r1 = n - 1 - r0, n - 1 - r1
    return AxisTables(r0.astype(np.int32), r1.astype(np.int32), t)


def inverse_tables(n, s, reverse, n_out):
    """Tables that carry a conformed axis of length n_out back to the input axis of length n: input index a
    reads conformed index min(floor(r s + 0.5), n_out - 1), r = a or n - 1 - a when reversed; t = 0."""
    r = np.arange(int(n), dtype=np.float64)
    if reverse:
        r = int(n) - 1 - r
    idx = np.minimum(np.floor(r * float(s) + 0.5), n_out - 1).astype(np.int32)
    return AxisTables(idx, idx.copy(), np.zeros(int(n), dtype=np.float64))


@dataclass(frozen=True)
class Plan:
    """The map between a scan's grid and the pipeline's frame.
    perm[j]: the world axis input axis j runs along; flips[j]: input axis j is reversed; spacing[j]: its voxel
    size in mm (snapped); shape: the scan's; out_shape: the conformed volume's, in the pipeline's axis order.
    forward[w]: tables of conformed axis w (it reads input axis source[w]); inverse[j]: tables of input axis j
    (it reads conformed axis perm[j])."""
    perm: tuple
    flips: tuple
    spacing: tuple
    obliquity_deg: float
    shape: tuple
    out_shape: tuple
    source: tuple
    forward: tuple
    inverse: tuple
    axis_codes: str

    @property
    def resamples(self):
        return any(s != 1.0 for s in self.spacing)

    @property
    def is_identity(self):
        return self.perm == (0, 1, 2) and not any(self.flips) and not self.resamples

    def describe(self):
        if self.is_identity:
            return "conform: identity"
        sp = ", ".join(f"{s:g}" for s in self.spacing)
        return f"conform: {self.axis_codes} -> LPS, spacing ({sp}) mm, obliquity {self.obliquity_deg:.1f}°"


def plan(affine, shape):
    """The Plan of a scan with voxel-to-world transform `affine` (4x4) and array shape `shape` (X, Y, Z)."""
    affine = np.asarray(affine, dtype=np.float64)
    shape = tuple(int(n) for n in shape)
    if affine.shape != (4, 4) or len(shape) != 3 or any(n < 1 for n in shape):
        raise ValueError(f"conform.plan takes a 4x4 affine and a 3-D shape, got {affine.shape} and {shape}")
    R = affine[:3, :3]
    s = np.sqrt((R * R).sum(axis=0))
    if not (np.all(np.isfinite(R)) and np.all(np.isfinite(s)) and np.all(s > 0)):
        raise ValueError(f"affine gives voxel spacings {tuple(s)}: each must be finite and positive")
    C = R / s
    best, perm = -1.0, None
    for p in itertools.permutations(range(3)):          # lexicographic order: a tie keeps the smallest
        score = sum(abs(C[p[j], j]) for j in range(3))
        if score > best + 1e-12:
            best, perm = score, p
    picked = np.array([C[perm[j], j] for j in range(3)])
    flips = tuple(bool(np.sign(picked[j]) != TARGET_SIGNS[perm[j]]) for j in range(3))
    obliquity = float(np.degrees(np.max(np.arccos(np.minimum(np.abs(picked), 1.0)))))
    spacing = tuple(1.0 if abs(v - 1.0) <= UNIT_SNAP else float(v) for v in s)
    source = tuple(perm.index(w) for w in range(3))
    forward = tuple(forward_tables(shape[j], spacing[j], flips[j]) for j in source)
    out_shape = tuple(tb.n_out for tb in forward)
    inverse = tuple(inverse_tables(shape[j], spacing[j], flips[j], out_shape[perm[j]]) for j in range(3))
    codes = "".join(_LETTERS[perm[j]][1 if picked[j] > 0 else 0] for j in range(3))
    return Plan(tuple(perm), flips, spacing, obliquity, shape, out_shape, source, forward, inverse, codes)


def plan_for_modalities(affines, shapes):
    """One Plan for the modalities of a scan: they must share one shape, and their affines must agree within
    AFFINE_AGREEMENT per entry (ValueError otherwise).  The first modality's affine is the scan's."""
    shapes = [tuple(int(n) for n in s) for s in shapes]
    if any(s != shapes[0] for s in shapes):
        raise ValueError(f"modality volumes must share one shape, got {shapes}")
    first = np.asarray(affines[0], dtype=np.float64)
    for k, a in enumerate(affines[1:], start=1):
        gap = float(np.max(np.abs(np.asarray(a, dtype=np.float64) - first)))
        if not gap <= AFFINE_AGREEMENT:
            raise ValueError(f"the affines of modality 0 and modality {k} disagree by {gap:g} (limit {AFFINE_AGREEMENT:g})")
    return plan(first, shapes[0])


def conformed_affine(plan, affine):
    """The 4x4 that takes an index (i, j, k) of the conformed volume to world mm, for the scan whose header holds
    `affine` and whose Plan is `plan`.  Conformed axis w reads input axis j = plan.source[w] at i / spacing[j], or at
    (n_j - 1) - i / spacing[j] when the axis is reversed (forward_tables); the scan's own affine does the rest."""
    affine = np.asarray(affine, dtype=np.float64)
    if affine.shape != (4, 4):
        raise ValueError(f"conformed_affine takes a 4x4 affine, got {affine.shape}")
    to_input = np.zeros((4, 4), dtype=np.float64)
    to_input[3, 3] = 1.0
    for w in range(3):
        j = plan.source[w]
        if plan.flips[j]:
            to_input[j, w] = -1.0 / plan.spacing[j]
            to_input[j, 3] = float(plan.shape[j] - 1)
        else:
            to_input[j, w] = 1.0 / plan.spacing[j]
    return affine @ to_input


# ---- device side -------------------------------------------------------------------------------------------------

def _require_cuda_tensor(volume, what):
    import torch

    from . import _lib

    if not isinstance(volume, torch.Tensor):
        raise _lib.GtsError(f"{what} takes a torch tensor")
    if not volume.is_cuda:
        _lib.require_device(volume)                     # raises: there is no CPU route


def _gather(volume, axes, tables, mode, what):
    """volume: CUDA tensor [C, Z, Y, X] or [Z, Y, X] (x fastest).  Output axis k (0 = x) reads input axis axes[k]
    by tables[k].  Returns the gathered tensor with the same number of leading axes."""
    launch, out = _bind(volume, axes, tables, mode, what)
    launch()
    return out


def _bind(volume, axes, tables, mode, what):
    """(launch, out): the tables uploaded and the output allocated; launch() enqueues the kernel on the current
    stream (the measurement tool times it alone)."""
    import torch

    from . import _lib
    from ._volume import I16, SCAN_CODES

    _require_cuda_tensor(volume, what)
    if volume.dim() not in (3, 4) or volume.numel() == 0:
        raise _lib.GtsError(f"{what} takes a non-empty [C, Z, Y, X] or [Z, Y, X] volume, got {tuple(volume.shape)}")
    code = SCAN_CODES.get(volume.dtype)
    if code is None or (mode == MODE_NEAREST and code != I16):
        raise _lib.GtsError(f"{what}: dtype {volume.dtype} is not supported")
    volume = volume.contiguous()
    channels = volume.shape[0] if volume.dim() == 4 else 1
    Z, Y, X = (int(n) for n in volume.shape[-3:])
    in_dims = (X, Y, Z)
    for k in range(3):
        tb = tables[k]
        n = in_dims[axes[k]]
        if tb.n_out < 1 or min(tb.idx0.min(), tb.idx1.min()) < 0 or max(tb.idx0.max(), tb.idx1.max()) >= n:
            raise _lib.GtsError(f"{what}: the plan does not fit a volume of shape {in_dims}")
    out_dims = tuple(tables[k].n_out for k in range(3))
    dev = volume.device
    idx = np.concatenate([np.concatenate([tb.idx0 for tb in tables]), np.concatenate([tb.idx1 for tb in tables])])
    idx_dev = torch.from_numpy(idx.astype(np.int32)).to(dev)
    t_dev = torch.from_numpy(np.concatenate([tb.t for tb in tables]).astype(np.float64)).to(dev)
    total = sum(out_dims)
    out_dtype = torch.float32 if mode == MODE_TRILINEAR else volume.dtype
    lead = (channels,) if volume.dim() == 4 else ()
    out = torch.empty(lead + out_dims[::-1], dtype=out_dtype, device=dev)
    lib = _lib.load()

    def launch():
        _lib.check(lib.gts_conform_gather(volume.data_ptr(), code, channels, X, Y, Z, axes[0], axes[1], axes[2],
                                          out_dims[0], out_dims[1], out_dims[2], idx_dev.data_ptr(),
                                          idx_dev[total:].data_ptr(), t_dev.data_ptr(), mode, out.data_ptr(),
                                          _lib.current_stream()), "gts_conform_gather")
    return launch, out


def _check_shape(volume, shape, what):
    from . import _lib

    got = tuple(int(n) for n in volume.shape[-3:])[::-1] if hasattr(volume, "shape") and len(volume.shape) >= 3 else None
    if got != tuple(shape):
        raise _lib.GtsError(f"{what}: volume of shape {got} (x, y, z), the plan is for {tuple(shape)}")


def conform_scan(staged, plan):
    """The scan in the pipeline's frame: device tensor [C, OZ, OY, OX].  staged: CUDA tensor [C, Z, Y, X] (int16
    or float32) on the scan's own grid.  Pure reorientation keeps the dtype bit for bit; any other plan gives
    trilinear float32.  An identity plan returns `staged` itself."""
    _check_shape(staged, plan.shape, "conform_scan")
    if plan.is_identity:
        _require_cuda_tensor(staged, "conform_scan")
        return staged
    mode = MODE_TRILINEAR if plan.resamples else MODE_EXACT
    return _gather(staged, plan.source, plan.forward, mode, "conform_scan")


def conform_labels(volume, plan):
    """An int16 label volume on the scan's grid -> the pipeline's frame, nearest neighbour."""
    _check_shape(volume, plan.shape, "conform_labels")
    return _gather(volume, plan.source, plan.forward, MODE_NEAREST, "conform_labels")


def unconform_labels(volume, plan, z_fastest=False):
    """An int16 label volume in the pipeline's frame -> the scan's own grid [.., Z, Y, X], nearest neighbour.
    z_fastest: `volume` is a C-order [X, Y, Z] tensor, the layout the prediction kernels write, and not
    [Z, Y, X]; the gather absorbs the change of layout."""
    if z_fastest:
        if len(volume.shape) != 3 or tuple(int(n) for n in volume.shape) != tuple(plan.out_shape):
            from . import _lib

            raise _lib.GtsError(f"unconform_labels: volume {tuple(volume.shape)}, the plan gives {plan.out_shape}")
        axes = tuple(2 - w for w in plan.perm)          # conformed axis w is memory axis 2 - w of a C-order [X, Y, Z]
    else:
        _check_shape(volume, plan.out_shape, "unconform_labels")
        axes = plan.perm
    return _gather(volume, axes, plan.inverse, MODE_EXACT, "unconform_labels")
