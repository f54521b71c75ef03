"""Refinement-CNN training, host side (no GPU): PredLogitDataset, collate_refinement_net, the CLI's flags,
progress file and folds, and argument errors of the conv3d entry points (C1-C5)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import cnn_data


def test_modules_import():
    from model.cnn_model import RefinementModel  # noqa: F401
    import scripts.train_refinement_cnn  # noqa: F401


def test_pred_logit_dataset_reads_and_caches_the_crop(tmp_path, monkeypatch):
    from data_processing import data_loader
    from data_processing.image_processing import determine_tumor_crop

    cnn_data.write(str(tmp_path / "d"), str(tmp_path / "l"), ["BraTS_a"])
    ds = data_loader.PredLogitDataset(str(tmp_path / "l"))
    logits, crop = ds.get_one("BraTS_a")
    want = cnn_data.make(100)[2]
    assert logits.dtype == np.float32 and np.array_equal(logits, want)
    ref = determine_tumor_crop(np.argmax(want, axis=-1))
    assert all(np.array_equal(a, b) for a, b in zip(crop, ref))
    # the second read takes the cached crop: determine_tumor_crop is not called again
    monkeypatch.setattr(data_loader, "determine_tumor_crop", lambda *_: pytest.fail("crop recomputed"))
    _, again = ds.get_one("BraTS_a")
    assert again is crop
    with pytest.raises(FileNotFoundError):
        ds.get_one("BraTS_missing")


def test_image_dataset_yields_mri_image_label_and_collate(tmp_path):
    from data_processing.data_loader import ImageGraphDataset, collate_refinement_net

    cnn_data.write(str(tmp_path / "d"), str(tmp_path / "l"), ["BraTS_a"])
    ds = ImageGraphDataset(str(tmp_path / "d") + os.sep, "BraTS", read_graph=False, read_image=True, read_label=True)
    mri, img, lab = ds[0]
    want_img, want_lab, _ = cnn_data.make(100)
    assert mri == "BraTS_a" and np.array_equal(img, want_img) and np.array_equal(lab, want_lab)
    m, t_img, t_lab = collate_refinement_net([ds[0]])
    assert m == mri and t_img.dtype == torch.float32 and t_lab.dtype == torch.int64
    assert torch.equal(t_img, torch.from_numpy(want_img)) and torch.equal(t_lab, torch.from_numpy(want_lab).long())


def test_cli_flags_and_defaults_match_the_reference():
    from scripts.train_refinement_cnn import build_parser

    p = build_parser()
    flags = {a.option_strings[0]: a for a in p._actions if a.option_strings and a.dest != "help"}
    assert sorted(flags) == ["-d", "-k", "-l", "-o", "-p", "-r", "-x"]
    want = {"-d": ("data_dir", None), "-l": ("saved_logit_dir", None), "-o": ("output_dir", None),
            "-r": ("run_name", None), "-k": ("num_folds", 5), "-p": ("data_prefix", ""),
            "-x": ("random_hyperparams", False)}
    for flag, (dest, default) in want.items():
        assert flags[flag].dest == dest and flags[flag].default == default
    assert flags["-r"].required
    args = p.parse_args(["-r", "run", "-k", "1", "-x"])
    assert args.num_folds == 1 and args.random_hyperparams
    with pytest.raises(SystemExit):
        p.parse_args([])


def test_progress_file_format(tmp_path, capsys):
    from scripts.train_refinement_cnn import document_metrics
    from utils.hyperparam_helpers import populate_hardcoded_hyperparameters
    from utils.training_helpers import create_run_progress_file

    fp = str(tmp_path / "run.txt")
    create_run_progress_file(fp, "CNN", populate_hardcoded_hyperparameters("CNN"))
    document_metrics(fp, "run_f1_val", np.array([0.123456, 0.9, 0.8, 0.7, 1.5, 2.5, 3.5]))
    lines = open(fp).read().splitlines()
    assert lines[:3] == ["----Model Parameters----", "Model\tCNN", "Epochs\t1"]
    assert lines[-3:-1] == ["Fold\tLoss\tWT_Dice\tCT_Dice\tET_Dice", ""]
    assert lines[-1] == "run_f1_val\t0.1235\t0.9\t0.8\t0.7"
    out = capsys.readouterr().out
    assert "#run_f1_val Results#" in out and "WT HD95: 1.5, CT HD95: 2.5, ET HD95: 3.5" in out


def test_fold_assignment_holds_out_each_chunk():
    from scripts.train_refinement_cnn import fold_splits

    folds = fold_splits(7, 3)
    assert [v for _, v in folds] == [[0, 1], [2, 3], [4, 5]]
    assert folds[0][0] == [2, 3, 4, 5, 6] and folds[2][0] == [0, 1, 2, 3, 6]
    for train, val in folds:
        assert not set(train) & set(val) and all(isinstance(i, int) for i in train)


def test_conv3d_entry_points_reject_bad_arguments_without_a_gpu(hip_lib):
    one = ctypes.c_void_p(256)
    big = 1 << 40
    ws = hip_lib.gts_conv3d_fwd_workspace(8, 16)
    assert ws == 125 * 2 * 64 * 4
    fwd, dat, wgt = hip_lib.gts_conv3d_fwd_f32, hip_lib.gts_conv3d_bwd_data_f32, hip_lib.gts_conv3d_bwd_weight_f32
    assert fwd(None, one, one, one, 4, 4, 4, 8, 16, 1, one, ws, None) == -1
    for cin, cout in ((0, 16), (33, 16), (8, 0), (8, 33)):               # unsupported channel counts
        assert fwd(one, one, one, one, 4, 4, 4, cin, cout, 1, one, big, None) == -2
        assert dat(one, one, one, one, 4, 4, 4, cin, cout, one, big, None) == -2
        assert wgt(one, one, one, one, 4, 4, 4, cin, cout, one, big, None) == -2
    for dims in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (-1, 4, 4), (4096, 4096, 4096)):   # zero / huge dimensions
        assert fwd(one, one, one, one, *dims, 8, 16, 1, one, big, None) == -2
        assert dat(one, one, one, one, *dims, 16, 4, one, big, None) == -2
        assert wgt(one, one, one, one, *dims, 8, 16, one, big, None) == -2
    assert fwd(one, one, one, one, 4, 4, 4, 8, 16, 2, one, big, None) == -3          # relu flag
    # short workspace
    assert fwd(one, one, one, one, 4, 4, 4, 8, 16, 1, one, ws - 1, None) == -2
    need = hip_lib.gts_conv3d_bwd_data_workspace(4, 4, 4, 16, 4)
    assert need > 0 and dat(one, one, None, one, 4, 4, 4, 16, 4, one, need - 1, None) == -2
    need = hip_lib.gts_conv3d_bwd_weight_workspace(4, 4, 4, 8, 16)
    assert need > 0 and wgt(one, one, one, None, 4, 4, 4, 8, 16, one, need - 1, None) == -2
    assert hip_lib.gts_conv3d_bwd_weight_workspace(0, 4, 4, 8, 16) == 0


def test_python_layer_refuses_cpu_tensors():
    from gts import _lib
    from gts.conv3d import refinement_logits
    from model.networks import CnnRefinementNet

    with pytest.raises(_lib.GtsError):
        refinement_logits(torch.zeros(4, 4, 4, 8), CnnRefinementNet(8, 4, [16]))


def test_prefetch_thread_ends_when_the_consumer_stops_early():
    import threading

    from model.cnn_model import RefinementModel

    class Logits:
        def get_one(self, mri):
            return np.zeros((2, 2, 2, 4), np.float32), np.ix_(range(2), range(2), range(2))

    model = RefinementModel.__new__(RefinementModel)
    model.prefetch, model.logit_dataset = True, Logits()
    endless = ((f"m{i}", np.zeros((2, 2, 2, 4), np.float32), np.zeros((2, 2, 2), np.int16)) for i in range(10 ** 9))
    gen = model._samples(endless)
    x, y = next(gen)
    assert tuple(x.shape) == (2, 2, 2, 8) and tuple(y.shape) == (8,)
    gen.close()          # the consumer leaves after one sample
    assert not any(t.name == "gts-cnn-prefetch" for t in threading.enumerate())
