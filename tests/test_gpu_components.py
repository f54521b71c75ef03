"""gts.components on the MI355X against scipy.ndimage.label (tests/components_ref.py): the roots, the
filtered volumes and the four stats, all compared for equality — everything is integer."""
import numpy as np
import pytest
import torch

from tests import components_ref as ref

pytestmark = pytest.mark.gpu
CONNECTIVITIES = (6, 26)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _roots(labels, connectivity):
    from gts import components

    return components.component_roots(_dev(labels), connectivity).cpu().numpy()


def _check_roots(labels, connectivity):
    return ref.check_roots(_roots(labels, connectivity), labels, connectivity)


def _check_filter(labels, min_voxels, connectivity, **et):
    """Device filter == ref_filter, volume and stats; returns (volume, stats list)."""
    from gts import components

    got, stats = components.remove_small_components(_dev(labels), min_voxels, connectivity, **et)
    want, want_stats = ref.ref_filter(labels, min_voxels, connectivity, **et)
    assert got.dtype == torch.int16 and tuple(got.shape) == labels.shape
    assert stats.is_cuda and stats.dtype == torch.int64
    assert np.array_equal(got.cpu().numpy(), want)
    assert stats.cpu().tolist() == want_stats
    return want, want_stats


def _bernoulli(shape, p, rng):
    return ((rng.random(shape) < p) * rng.integers(1, 4, shape)).astype(np.int16)


# 1. random volumes around the site-percolation thresholds (0.31 at 6 neighbours, 0.10 at 26)
@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
@pytest.mark.parametrize("shape", [(37, 50, 61), (129, 3, 70), (5, 90, 33), (16, 16, 16), (1, 1, 90), (64, 80),
                                   (1, 40, 33, 21)])
def test_random_volumes_around_percolation(hip_lib, shape, connectivity):
    rng = np.random.default_rng(sum(shape) + connectivity)
    for p in (0.05, 0.10, 0.20, 0.31, 0.45, 0.7):
        labels = _bernoulli(shape, p, rng)
        _check_roots(labels, connectivity)
        _check_filter(labels, 4, connectivity)


def _serpentine(dims, offset=(0, 0, 0), shape=(24, 24, 24)):
    """A one-voxel-wide path through every second line (even x, even y) of a box of `dims` at `offset`:
    full lines along Z joined at alternating ends, planes joined at the end of their last line."""
    a, b, c = dims
    box = np.zeros(dims, dtype=np.int16)
    joints = 0

    def end():
        nonlocal joints
        joints += 1
        return 0 if joints % 2 else c - 1

    xs = list(range(0, a, 2))
    for k, x in enumerate(xs):
        ys = list(range(0, b, 2))
        if k % 2:
            ys.reverse()
        for j, y in enumerate(ys):
            box[x, y, :] = 1
            if j + 1 < len(ys):
                box[x, (y + ys[j + 1]) // 2, end()] = 1
        if k + 1 < len(xs):
            box[x + 1, ys[-1], end()] = 1
    vol = np.zeros(shape, dtype=np.int16)
    vol[tuple(slice(o, o + d) for o, d in zip(offset, dims))] = box
    return vol


def _spiral(n=24):
    """A square spiral with one-voxel walls in the plane x = 5."""
    plane = np.zeros((n, n), dtype=bool)
    y, z, dy, dz = 0, 0, 0, 1
    plane[y, z] = True
    while True:
        ny, nz = y + dy, z + dz
        ahead = (ny + dy, nz + dz)
        blocked = not (0 <= ny < n and 0 <= nz < n) or plane[ny, nz] or \
            (0 <= ahead[0] < n and 0 <= ahead[1] < n and plane[ahead])
        if blocked:
            dy, dz = dz, -dy
            ny, nz = y + dy, z + dz
            ahead = (ny + dy, nz + dz)
            if not (0 <= ny < n and 0 <= nz < n) or plane[ny, nz] or \
                    (0 <= ahead[0] < n and 0 <= ahead[1] < n and plane[ahead]):
                break
        y, z = ny, nz
        plane[y, z] = True
    vol = np.zeros((n, n, n), dtype=np.int16)
    vol[5] = plane * 3
    return vol


# 2. long union chains
@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
def test_long_chains(hip_lib, connectivity):
    snake = _serpentine((24, 24, 24))
    assert snake.sum() > 24 * 12 * 12
    assert _check_roots(snake, connectivity) == 1
    spiral = _spiral()
    assert spiral[5].sum() > 200
    assert _check_roots(spiral, connectivity) == 1
    # two paths whose boxes touch only along the edge x = 11 | 12, z = 11 | 12
    pair = _serpentine((11, 24, 12), (1, 0, 0)) + _serpentine((11, 24, 12), (12, 0, 12))
    assert pair[11, 0, 11] and pair[12, 0, 12] and pair.max() == 1
    assert _check_roots(pair, connectivity) == (2 if connectivity == 6 else 1)
    _check_filter(pair, int(pair.sum()), connectivity)


# 3. checkerboard by coordinate parity
def test_checkerboard(hip_lib):
    shape = (17, 18, 19)
    x, y, z = np.indices(shape)
    board = (((x + y + z) % 2 == 0) * 2).astype(np.int16)
    n_fg = int((board != 0).sum())
    assert _check_roots(board, 6) == n_fg
    assert np.array_equal(_roots(board, 6)[board != 0], np.flatnonzero(board.ravel()) + 1)
    assert _check_roots(board, 26) == 1
    _, stats = _check_filter(board, 2, 6)
    assert stats == [n_fg, n_fg, n_fg, 0]


# 4. seams of runs, waves and grids
@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
@pytest.mark.parametrize("z_extent", [63, 64, 65, 127, 129])
def test_contiguous_extent_seams(hip_lib, z_extent, connectivity):
    rng = np.random.default_rng(z_extent)
    for shape in [(2, 9, z_extent), (9, 2, z_extent)]:
        for p in (0.5, 0.9, 1.0):
            labels = _bernoulli(shape, p, rng)
            _check_roots(labels, connectivity)
            _check_filter(labels, 5, connectivity)


@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_plates_and_bars_across_tile_multiples(hip_lib, axis, connectivity):
    shape = [5, 6, 7]
    shape[axis] = 70                                     # crosses 8, 16, 32 and 64
    vol = np.zeros(shape, dtype=np.int16)
    bar = [1, 1, 1]
    bar[axis] = slice(None)
    vol[tuple(bar)] = 1                                  # a bar along the axis
    plate = [slice(None)] * 3
    plate[(axis + 1) % 3] = 4                            # a one-voxel plate holding the axis
    vol[tuple(plate)] = 2
    far = [3, 3, 3]
    far[axis] = slice(9, 66)
    far[(axis + 1) % 3] = 2                              # a second bar, two voxels from the first
    vol[tuple(far)] = 3
    _check_roots(vol, connectivity)
    _check_filter(vol, 60, connectivity)
    wide = np.zeros((70, 70, 70), dtype=np.int16)        # the same crossings with more than one block per plane
    wide[tuple(bar)] = 1
    wide[tuple(plate)] = 2
    wide[69, 69, 69] = 1
    assert _check_roots(wide, connectivity) == 3
    _check_filter(wide, 2, connectivity)


# 5. extremes
@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
def test_extremes(hip_lib, connectivity):
    shape = (9, 10, 11)
    full = np.full(shape, 3, dtype=np.int16)
    assert _check_roots(full, connectivity) == 1
    out, stats = _check_filter(full, full.size, connectivity)
    assert stats == [1, 0, 0, 0] and np.array_equal(out, full)
    assert _check_filter(full, full.size + 1, connectivity)[1] == [1, 1, full.size, 0]
    empty = np.zeros(shape, dtype=np.int16)
    assert _check_roots(empty, connectivity) == 0
    out, stats = _check_filter(empty, 100, connectivity)
    assert stats == [0, 0, 0, 0] and not out.any()
    corners = np.zeros(shape, dtype=np.int16)
    corners[::shape[0] - 1, ::shape[1] - 1, ::shape[2] - 1] = 1
    assert _check_roots(corners, connectivity) == 8
    assert _check_filter(corners, 2, connectivity)[1] == [8, 8, 8, 0]
    one = np.zeros(shape, dtype=np.int16)
    one[4, 5, 6] = 2
    assert _check_roots(one, connectivity) == 1
    lone = np.ones((1, 1, 1), dtype=np.int16)
    assert _check_roots(lone, connectivity) == 1
    assert _check_filter(lone, 2, connectivity)[1] == [1, 1, 1, 0]


def _boxes():
    """Isolated boxes of 26, 27 and 28 voxels, the 27 made of labels 1, 2 and 3."""
    vol = np.zeros((20, 9, 9), dtype=np.int16)
    vol[1:4, 1:4, 1:4] = 1
    vol[1, 1, 1] = 0                                      # 26
    vol[7:10, 1:4, 1:4] = 1
    vol[8, 1:4, 1:4] = 2
    vol[9, 1:4, 1:4] = 3                                  # 27
    vol[13:16, 1:4, 1:4] = 1
    vol[16, 2, 2] = 1                                     # 28
    return vol


# 6. threshold edges
@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
def test_threshold_edges(hip_lib, connectivity):
    from gts import components

    vol = _boxes()
    out, stats = _check_filter(vol, 27, connectivity)
    assert stats == [3, 1, 26, 0]
    assert not out[1:4].any() and np.array_equal(out[5:], vol[5:])          # the mixed box counts once, labels kept
    for none in (0, 1):
        out, stats = _check_filter(vol, none, connectivity)
        assert stats == [3, 0, 0, 0] and np.array_equal(out, vol)
    odd = vol.copy()
    odd[odd == 2] = -1
    odd[odd == 3] = 4
    out, stats = _check_filter(odd, 27, connectivity)
    assert stats == [3, 1, 26, 0] and (out == -1).sum() == 9 and (out == 4).sum() == 9
    labels = _dev(vol)
    same, stats = components.remove_small_components(labels, 27, connectivity, out=labels)
    assert same is labels and stats.cpu().tolist() == [3, 1, 26, 0]
    assert np.array_equal(labels.cpu().numpy(), ref.ref_filter(vol, 27, connectivity)[0])


def _tumour(n_et, island_et=0):
    """An edema block with n_et enhancing voxels inside, and a far island of island_et enhancing voxels."""
    vol = np.zeros((16, 16, 40), dtype=np.int16)
    vol[2:10, 2:10, 2:12] = 2
    et = np.zeros(8 * 8 * 10, dtype=bool)
    et[:n_et] = True
    vol[2:10, 2:10, 2:12][et.reshape(8, 8, 10)] = 4
    vol[13, 13, 20:20 + island_et] = 4
    return vol


# 7. the enhancing-tumour rule
@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
def test_enhancing_rule(hip_lib, connectivity):
    et = dict(et_label=4, et_min_voxels=50, et_replacement=1)
    out, stats = _check_filter(_tumour(49), 0, connectivity, **et)
    assert stats == [1, 0, 0, 49] and (out == 1).sum() == 49 and not (out == 4).any()
    out, stats = _check_filter(_tumour(50), 0, connectivity, **et)
    assert stats == [1, 0, 0, 0] and (out == 4).sum() == 50
    out, stats = _check_filter(_tumour(0), 0, connectivity, **et)
    assert stats == [1, 0, 0, 0] and np.array_equal(out, _tumour(0))
    # 45 + 10 enhancing voxels; rule (a) removes the island first, the 45 left are below 50
    out, stats = _check_filter(_tumour(45, 10), 20, connectivity, **et)
    assert stats == [2, 1, 10, 45] and (out == 1).sum() == 45 and not (out == 4).any()
    out, stats = _check_filter(_tumour(45, 10), 5, connectivity, **et)
    assert stats == [2, 0, 0, 0] and (out == 4).sum() == 55
    # the rule switched off, and no ET labels given
    assert _check_filter(_tumour(3), 0, connectivity, et_label=4, et_min_voxels=0, et_replacement=1)[1] == [1, 0, 0, 0]
    assert _check_filter(_tumour(3), 0, connectivity)[1] == [1, 0, 0, 0]


# 8. BraTS size, once: blobs plus 0.1 % salt noise; two runs must agree to the bit
@pytest.mark.timeout(120)
def test_brats_size_and_determinism(hip_lib):
    from gts import components, synth_mri

    labels = synth_mri.make_prediction(8, (240, 240, 155), salt=0.001)
    assert labels.shape == (240, 240, 155) and (labels == 4).sum() > 8000
    dev = _dev(labels)
    et = dict(et_label=4, et_min_voxels=10 ** 7, et_replacement=1)
    for connectivity in CONNECTIVITIES:
        roots = components.component_roots(dev, connectivity)
        again = components.component_roots(dev, connectivity)
        assert torch.equal(roots, again)
        k = ref.check_roots(roots.cpu().numpy(), labels, connectivity)
        assert k > 1000
        out, stats = components.remove_small_components(dev, 50, connectivity, **et)
        out2, stats2 = components.remove_small_components(dev, 50, connectivity, **et)
        assert torch.equal(out, out2) and torch.equal(stats, stats2)
        want, want_stats = ref.ref_filter(labels, 50, connectivity, **et)
        assert np.array_equal(out.cpu().numpy(), want) and stats.cpu().tolist() == want_stats
        assert want_stats[1] > 1000 and want_stats[3] > 0


def test_wrappers_on_the_device(hip_lib):
    from gts import GtsError, components

    with pytest.raises(GtsError, match="empty"):
        components.component_roots(torch.zeros((0, 3, 3), dtype=torch.int16, device="cuda"))
    with pytest.raises(GtsError, match="at most 3"):
        components.component_roots(torch.zeros((2, 2, 2, 2), dtype=torch.int16, device="cuda"))
    with pytest.raises(GtsError, match="out must be"):
        components.remove_small_components(_dev(_boxes()), 5, out=torch.zeros(3, dtype=torch.int16, device="cuda"))
    # a non-contiguous view is taken as the volume it shows; the work runs on the current stream
    vol = _boxes()
    view = _dev(np.ascontiguousarray(vol.transpose(2, 1, 0))).permute(2, 1, 0)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        out, stats = components.remove_small_components(view, 27, 6)
    stream.synchronize()
    assert np.array_equal(out.cpu().numpy(), ref.ref_filter(vol, 27, 6)[0]) and stats.cpu().tolist() == [3, 1, 26, 0]


# 9. the CLIs.  One process runs every variant, so the nets, the scan and the graph are the same in all of them.
CLEANUP = ["--min_component_voxels", "300", "--min_enhancing_voxels", "100000000"]


def _run(module, argv):
    import io
    from contextlib import redirect_stdout

    with redirect_stdout(io.StringIO()) as log:
        rc = module.main(argv)
    assert not rc, log.getvalue()[-2000:]
    return log.getvalue()


def _bytes(path):
    with open(path, "rb") as f:
        return f.read()


def _check_cli_outputs(read, plain, zeros, by_connectivity, logs, ids, min_voxels=300):
    """plain / zeros / by_connectivity[c]: output folders of the run without the flags, with the flags at 0,
    and with CLEANUP (or another min_voxels) at connectivity c; the filtered files must be ref_filter of the
    plain ones."""
    import os

    for sid in ids:
        name = f"{sid}.nii.gz"
        assert _bytes(os.path.join(zeros, name)) == _bytes(os.path.join(plain, name))
        base = read(os.path.join(plain, name))
        assert base.dtype == np.int16 and base.shape == (240, 240, 155)
        for connectivity, folder in by_connectivity.items():
            want, stats = ref.ref_filter(base, min_voxels, connectivity, et_label=4, et_min_voxels=10 ** 8, et_replacement=1)
            assert np.array_equal(read(os.path.join(folder, name)), want), (sid, connectivity)
            line = [ln for ln in logs[connectivity].splitlines() if ln.startswith(f"{sid}:")]
            note = ", ".join(f"{k} {v}" for k, v in zip(("components", "components_removed", "voxels_removed",
                                                         "et_relabelled"), stats))
            assert len(line) == 1 and note in line[0], (line, note)


@pytest.mark.timeout(300)
def test_segment_scans_writes_the_filtered_volume(hip_lib, tmp_path):
    import os
    import sys

    from data_processing import nifti_io
    from gts import synth_mri
    from model.networks import init_graph_net
    from scripts import segment_scans
    from utils.hyperparam_helpers import EvalParamSet

    raw = str(tmp_path / "raw")
    synth_mri.write_sample(raw, "BraTS_000", 300)
    torch.manual_seed(0)
    gnn = str(tmp_path / "gnn.pt")
    torch.save(init_graph_net("GSpool", EvalParamSet(20, 4, [256] * 4, None, None)).state_dict(), gnn)
    base = ["-d", raw, "-g", gnn, "-n", "6000"]
    sys.modules.pop("gts.components", None)
    plain, zeros = str(tmp_path / "plain"), str(tmp_path / "zeros")
    assert "BraTS_000: done\n" in _run(segment_scans, base + ["-o", plain])
    _run(segment_scans, base + ["-o", zeros, "--min_component_voxels", "0", "--connectivity", "6",
                                "--min_enhancing_voxels", "0"])
    assert "gts.components" not in sys.modules                    # the defaults never reach the new code
    folders, logs = {}, {}
    for connectivity in CONNECTIVITIES:
        folders[connectivity] = str(tmp_path / f"c{connectivity}")
        logs[connectivity] = _run(segment_scans, base + ["-o", folders[connectivity], "--connectivity",
                                                         str(connectivity)] + CLEANUP)
    _check_cli_outputs(nifti_io.read_nifti_raw, plain, zeros, folders, logs, ["BraTS_000"])
    # an untrained net may predict one connected mass, which 300 voxels never touch: a limit above the volume's
    # size must empty the file, whatever was predicted
    everything = str(tmp_path / "everything")
    log = _run(segment_scans, base + ["-o", everything, "--min_component_voxels", str(10 ** 7)])
    _check_cli_outputs(nifti_io.read_nifti_raw, plain, zeros, {26: everything}, {26: log}, ["BraTS_000"], 10 ** 7)
    assert not nifti_io.read_nifti_raw(os.path.join(everything, "BraTS_000.nii.gz")).any()


@pytest.mark.timeout(300)
def test_generate_gnn_predictions_writes_the_filtered_volume(hip_lib, tmp_path):
    import sys

    from data_processing import nifti_io
    from model.networks import init_graph_net
    from scripts import generate_gnn_predictions
    from tests.dataset_util import write_dataset
    from utils.hyperparam_helpers import EvalParamSet

    data = str(tmp_path / "data") + "/"
    ids = sorted(write_dataset(data, 2))
    torch.manual_seed(0)
    gnn = str(tmp_path / "gnn.pt")
    torch.save(init_graph_net("GSpool", EvalParamSet(20, 4, [256] * 4, None, None)).state_dict(), gnn)
    base = ["-d", data, "-p", "BraTS_", "-w", gnn, "-f", "preds"]
    sys.modules.pop("gts.components", None)
    plain, zeros = str(tmp_path / "plain"), str(tmp_path / "zeros")
    _run(generate_gnn_predictions, base + ["-o", plain])
    _run(generate_gnn_predictions, base + ["-o", zeros, "--min_component_voxels", "0", "--min_enhancing_voxels", "0"])
    assert "gts.components" not in sys.modules
    folders, logs = {}, {}
    for connectivity in CONNECTIVITIES:
        folders[connectivity] = str(tmp_path / f"c{connectivity}")
        logs[connectivity] = _run(generate_gnn_predictions, base + ["-o", folders[connectivity], "--connectivity",
                                                                    str(connectivity)] + CLEANUP)
    _check_cli_outputs(lambda fp: nifti_io.read_nifti(fp, np.int16), plain, zeros, folders, logs, ids)
    with pytest.raises(ValueError, match="preds"):
        generate_gnn_predictions.main(["-d", data, "-p", "BraTS_", "-w", gnn, "-f", "logits", "-o", plain] + CLEANUP)


# 10. the CNN's crop box follows the surviving GNN prediction
class _FixedLogits:
    """Stands in for the graph net and its graph: the node logits are given."""

    def __init__(self, logits):
        self.logits = logits

    def to(self, device):
        return self

    def __call__(self, graph, feats):
        return self.logits


def test_crop_box_ignores_a_filtered_island(hip_lib):
    from data_processing.labels import INTERNAL_TO_BRATS
    from model.networks import CnnRefinementNet
    from scripts import cleanup
    from scripts import generate_joint_predictions as joint

    cube, grid = 4, 8                                      # 8^3 supervoxels of 4^3 voxels in a 32^3 volume
    ids = np.arange(grid ** 3, dtype=np.int16).reshape(grid, grid, grid)
    svs = np.repeat(np.repeat(np.repeat(ids, cube, 0), cube, 1), cube, 2)
    node_class = np.zeros((grid, grid, grid), dtype=np.int64)
    node_class[2:5, 1:4, 2:6] = 2                          # the blob: 36 supervoxels, voxels [8:20, 4:16, 8:24]
    node_class[3, 2, 3] = 3
    node_class[7, 7, 7] = 1                                # the island: one supervoxel of 64 voxels, far away
    logits = np.full((grid ** 3, 4), -1.0, dtype=np.float32)
    logits[np.arange(grid ** 3), node_class.ravel()] = 2.0
    svs_dev, logits_dev = _dev(svs), _dev(logits)
    blob_box = [list(range(7, 21)), list(range(3, 17)), list(range(7, 25))]          # the blob's box, dilated by one
    inflated = [list(range(7, 21)) + list(range(27, 32)), list(range(3, 17)) + list(range(27, 32)),
                list(range(7, 25)) + list(range(27, 32))]
    wanted = cleanup.Cleanup(min_component_voxels=65)
    assert [h.tolist() for h in joint.gnn_crop_box(svs_dev, logits_dev, wanted).host] == blob_box
    assert [h.tolist() for h in joint.gnn_crop_box(svs_dev, logits_dev).host] == inflated
    only_et = cleanup.Cleanup(min_enhancing_voxels=10)     # no component rule: the box is the usual one
    assert [h.tolist() for h in joint.gnn_crop_box(svs_dev, logits_dev, only_et).host] == inflated
    keeps = cleanup.Cleanup(min_component_voxels=64)       # the island has exactly 64 voxels: it stays
    assert [h.tolist() for h in joint.gnn_crop_box(svs_dev, logits_dev, keeps).host] == inflated
    import io
    from contextlib import redirect_stdout

    with redirect_stdout(io.StringIO()) as log:            # nothing survives: the empty-prediction rule, whole volume
        box = joint.gnn_crop_box(svs_dev, logits_dev, cleanup.Cleanup(min_component_voxels=10 ** 6))
    assert box.shape == (32, 32, 32) and "No GNN predicted tumor" in log.getvalue()

    torch.manual_seed(3)
    cnn = CnnRefinementNet(8, 4, [16]).cuda().eval()
    rng = np.random.default_rng(3)
    img = rng.standard_normal((32, 32, 32, 4)).astype(np.float32)
    relabel = torch.from_numpy(INTERNAL_TO_BRATS).cuda()
    net = _FixedLogits(logits_dev)
    feats = np.zeros((grid ** 3, 20), dtype=np.float32)
    got = joint.predict_one_sample(net, cnn, net, feats, img, svs, relabel, cleanup=wanted)
    assert got.dtype == np.int16 and got.shape == (32, 32, 32)
    assert not got[27:, 27:, 27:].any()                    # no voxel of the island, nor of its dilated box
    outside = np.ones(got.shape, dtype=bool)
    outside[np.ix_(*blob_box)] = False
    assert not got[outside].any()
    # the finished volume was filtered again: no component below the limit is left, and the stats say what went
    numbers, k = ref.ref_labels(got, 26)
    assert k == 0 or np.bincount(numbers.ravel())[1:].min() >= 65
    found, removed, voxels, relabelled = wanted.last_stats.cpu().tolist()
    assert found - removed == k and relabelled == 0 and (voxels > 0) == (removed > 0)
