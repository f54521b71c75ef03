"""Joint GNN + CNN training, host side (no GPU): argument errors of J1 / J2, the CLI's flags, the model's
refusal to run without a GPU, and what the host builds for J2 (inverse crop tables, per-node voxel lists)
against a numpy restatement."""
import ctypes

import numpy as np
import pytest
import torch


def test_modules_import():
    import scripts.train_joint  # noqa: F401
    from gts.joint import joint_refinement_logits  # noqa: F401
    from model.joint_model import JointModel  # noqa: F401


def test_entry_points_reject_bad_arguments_without_a_gpu(hip_lib):
    one = ctypes.c_void_p(256)
    j1, j2 = hip_lib.gts_crop_concat_rows_f32, hip_lib.gts_crop_concat_rows_bwd_f32
    good1 = dict(cx=2, cy=3, cz=4, dim_y=5, dim_z=6, n_rows=7, ci=4, ct=4)

    def call1(ptrs=(one,) * 8, **kw):
        a = dict(good1, **kw)
        return j1(*ptrs, a["cx"], a["cy"], a["cz"], a["dim_y"], a["dim_z"], a["n_rows"], a["ci"], a["ct"], None)

    for missing in (1, 3, 4, 5, 6, 7):                      # svs, bg_row, xs, ys, zs, out
        ptrs = [one] * 8
        ptrs[missing] = None
        assert call1(tuple(ptrs)) == -1
    assert call1((None,) + (one,) * 7) == -1                # an image is required when it has channels
    assert call1((None,) + (one,) * 7, cx=0, ci=0) == 0     # an empty crop touches nothing
    assert call1(cy=6) == -2 and call1(cz=7) == -2          # a box larger than the volume
    assert call1(cx=-1) == -2 and call1(n_rows=-1) == -2 and call1(ci=-1) == -2
    assert call1(ct=0) == -2 and call1(ct=65) == -2

    good2 = dict(cx=2, cy=3, cz=4, dim_x=5, dim_y=5, dim_z=6, n_rows=7, ci=0, ct=4)

    def call2(ptrs=(one,) * 7, **kw):
        a = dict(good2, **kw)
        return j2(*ptrs, a["cx"], a["cy"], a["cz"], a["dim_x"], a["dim_y"], a["dim_z"], a["n_rows"], a["ci"],
                  a["ct"], None)

    for missing in range(7):
        ptrs = [one] * 7
        ptrs[missing] = None
        assert call2(tuple(ptrs)) == -1
    assert call2(cx=6) == -2 and call2(cy=6) == -2 and call2(cz=7) == -2
    assert call2(cx=-1) == -2 and call2(n_rows=-1) == -2 and call2(ci=-1) == -2 and call2(dim_x=0) == -2
    assert call2(ct=0) == -2 and call2(ct=65) == -2
    assert call2(dim_x=2048, dim_y=2048, dim_z=2048) == -2  # voxel indices past int32
    assert call2((None,) * 7, n_rows=0) == 0                # no table rows: nothing to write


def test_cli_flags_and_fold_check():
    from scripts.train_joint import build_parser, main

    p = build_parser()
    flags = {a.option_strings[0]: a for a in p._actions if a.option_strings and a.dest != "help"}
    assert sorted(flags) == ["-c", "-d", "-g", "-k", "-m", "-o", "-p", "-r", "-w", "-x"]
    want = {"-d": ("data_dir", None), "-o": ("output_dir", None), "-r": ("run_name", None), "-k": ("num_folds", 5),
            "-p": ("data_prefix", ""), "-m": ("gnn_type", "GSpool"), "-g": ("gnn_weights", ""),
            "-c": ("cnn_weights", ""), "-w": ("gnn_loss_weight", 1.0), "-x": ("random_hyperparams", False)}
    for flag, (dest, default) in want.items():
        assert flags[flag].dest == dest and flags[flag].default == default
    args = p.parse_args(["-r", "run", "-k", "1", "-w", "0", "-m", "GSmean"])
    assert args.num_folds == 1 and args.gnn_loss_weight == 0.0 and args.gnn_type == "GSmean"
    with pytest.raises(SystemExit):
        p.parse_args([])
    with pytest.raises(ValueError, match="folds"):
        main(["-r", "run", "-k", "0", "-d", "nowhere", "-o", "nowhere"])
    with pytest.raises(ValueError, match="weight"):
        main(["-r", "run", "-k", "1", "-w", "-1", "-d", "nowhere", "-o", "nowhere"])


def test_model_needs_a_gpu(monkeypatch):
    from model.joint_model import JointModel
    from utils.hyperparam_helpers import populate_hardcoded_hyperparameters

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="needs an AMD GPU"):
        JointModel("GSpool", populate_hardcoded_hyperparameters("GSpool"), populate_hardcoded_hyperparameters("CNN"),
                   None)


def _partitioning(rng, shape, n_rows):
    """Ids below -1 (they wrap as numpy wraps them), -1 (background), ids >= n_rows and every row in between."""
    svs = rng.integers(-n_rows - 3, n_rows + 3, size=shape).astype(np.int16)
    svs[rng.random(shape) < 0.3] = -1
    return svs


@pytest.mark.parametrize("seed", range(6))
def test_voxel_lists_and_inverse_tables_give_the_adjoint_of_the_gather(seed):
    """The numpy restatement of J1 is `cat(table, bg)[svs][box]`; its adjoint in fp64 is np.add.at over the
    resolved rows.  Walking the host-built lists through the inverse tables, as J2 does, must visit exactly
    the same (row, crop voxel) pairs, in raster order inside every row."""
    from gts import ops

    rng = np.random.default_rng(seed)
    shape = tuple(int(s) for s in rng.integers(1, 9, 3))
    n_rows = int(rng.integers(1, 12))
    svs = _partitioning(rng, shape, n_rows)
    if seed == 0:
        svs[(svs == 0) | (svs == -(n_rows + 1))] = -1       # a row without any voxel
    idx = [np.flatnonzero(rng.random(n) < 0.5) for n in shape]
    idx = [i if len(i) else np.array([0]) for i in idx]
    box = ops.CropBox(*idx, shape, "cpu")
    inv = box.inverse_host()
    for table, ix, extent in zip(inv, idx, shape):
        assert table.dtype == np.int32 and table.shape == (extent,)
        assert np.array_equal(np.flatnonzero(table >= 0), ix) and np.array_equal(table[ix], np.arange(len(ix)))
    list_ptr, list_vox = ops.supervoxel_voxel_lists(svs, n_rows)
    assert list_ptr.dtype == np.int32 and list_vox.dtype == np.int32
    assert list_ptr[0] == 0 and list_ptr[-1] == len(list_vox) and len(list_ptr) == n_rows + 1
    # the rows numpy resolves: table_plus_bg[id]; an id outside [-(n_rows + 1), n_rows] has no row at all
    flat = svs.reshape(-1).astype(np.int64)
    resolved = np.where(flat < 0, flat + n_rows + 1, flat)
    for n in range(n_rows):
        mine = list_vox[list_ptr[n]:list_ptr[n + 1]]
        assert np.array_equal(mine, np.flatnonzero(resolved == n))          # ascending = raster order
    inside = (flat >= -(n_rows + 1)) & (flat < n_rows) & (flat != -1)
    assert len(list_vox) == int(inside.sum())
    # the adjoint on the crop
    ct = 3
    dx = rng.standard_normal(box.shape + (ct,))
    want = np.zeros((n_rows + 1, ct))
    cropped = np.where(inside, resolved, n_rows).reshape(shape)[box.as_ix()]
    np.add.at(want, cropped.reshape(-1), dx.reshape(-1, ct))
    got = np.zeros((n_rows, ct))
    for n in range(n_rows):
        for v in list_vox[list_ptr[n]:list_ptr[n + 1]]:
            x, y, z = np.unravel_index(v, shape)
            i, j, k = inv[0][x], inv[1][y], inv[2][z]
            if min(i, j, k) >= 0:
                got[n] += dx[i, j, k]
    assert np.allclose(got, want[:n_rows], rtol=0, atol=1e-12)
    if seed == 0:
        assert list_ptr[0] == list_ptr[1] and not got[0].any()


def test_python_layer_refuses_cpu_tensors_and_foreign_lists():
    from gts import _lib, ops
    from gts.joint import joint_refinement_logits
    from model.networks import CnnRefinementNet

    shape = (4, 4, 4)
    box = ops.CropBox(np.arange(4), np.arange(4), np.arange(4), shape, "cpu")
    svs = torch.zeros(shape, dtype=torch.int16)
    with pytest.raises(_lib.GtsError):
        ops.crop_concat_rows(torch.zeros(shape + (4,)), svs, torch.zeros(3, 4), torch.zeros(4), box)
    with pytest.raises(_lib.GtsError):
        joint_refinement_logits(torch.zeros(3, 4), torch.zeros(shape + (4,)), svs, box, torch.zeros(4),
                                CnnRefinementNet(8, 4, [16]))
    lists = ops.SupervoxelLists(np.zeros((4, 4, 5), dtype=np.int16), 3, "cpu")
    with pytest.raises(_lib.GtsError, match="another volume"):
        ops.crop_concat_rows_bwd(torch.zeros(64, 4), lists, box)
