"""The conform stage on the MI355X (gts/conform.py, csrc/gts_conform.hip) against tests/conform_ref.py, and
`segment_scans --conform` end to end on scans of other orientations and spacings."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import conform_ref as R

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "gnn-tumor-seg_amd")
DEV = "cuda"

# (1,1,1); odd; longer than a wave's row along x; across the 64-wide LDS tile's edge in both tiled axes of every
# permutation that moves x and a multiple of neither 32 nor 64
EXACT_SHAPES = [(1, 1, 1), (5, 6, 7), (65, 3, 18), (70, 37, 3), (72, 5, 67), (16, 4, 3)]
SPACINGS = [(1, 1, 2), (0.5, 0.5, 1), (1.2, 0.8, 3.0), (0.9375, 0.9375, 5)]
# orientations that move the fastest axis: x <-> y, x -> z -> y -> x, x <-> z, each with flips
MOVING = [((1, 0, 2), (1, -1, 1)), ((2, 0, 1), (-1, 1, -1)), ((2, 1, 0), (1, 1, -1)), ((1, 2, 0), (-1, -1, 1))]


def _dev(a):
    """[.., X, Y, Z] numpy -> device tensor [.., Z, Y, X] (x fastest), as intake.stage_scan lays a scan out."""
    lead = a.ndim - 3
    axes = list(range(lead)) + [lead + 2, lead + 1, lead]
    return torch.from_numpy(np.ascontiguousarray(np.transpose(a, axes))).to(DEV)


def _host(t):
    a = t.cpu().numpy()
    lead = a.ndim - 3
    return np.transpose(a, list(range(lead)) + [lead + 2, lead + 1, lead])


def _plan(shape, perm, signs, spacing=(1.0, 1.0, 1.0)):
    from gts import conform

    pl = conform.plan(R.make_affine(perm, signs, spacing, (4.0, -7.5, 11.0)), shape)
    assert pl.perm == tuple(perm) and pl.flips == R.flips_of(perm, signs)
    return pl


def _values(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    full = (4,) + tuple(shape)
    if dtype == np.int16:
        return rng.integers(-30000, 30001, full).astype(np.int16)
    v = (rng.uniform(-3e4, 3e4, full) * rng.choice([1.0, 1e-3, 1e-6], full)).astype(np.float32)
    v.flat[0] = -0.0
    return v


@pytest.mark.parametrize("shape", EXACT_SHAPES)
def test_exact_mode_all_48_orientations(hip_lib, shape):
    from gts import conform

    for dtype in (np.int16, np.float32):
        a = _values(shape, dtype, 1)
        src = _dev(a)
        for perm, signs in R.ORIENTATIONS:
            pl = _plan(shape, perm, signs)
            assert not pl.resamples
            got = conform.conform_scan(src, pl)
            if pl.is_identity:
                assert got is src
                continue
            want = R.reorient(a, perm, signs)
            assert got.dtype == src.dtype and tuple(got.shape) == (4,) + pl.out_shape[::-1]
            assert _host(got).tobytes() == want.tobytes(), (shape, dtype, perm, signs)


@pytest.mark.parametrize("shape", [(5, 6, 7), (70, 37, 3), (16, 8, 3)])
def test_labels_round_trip_all_48_orientations(hip_lib, shape):
    from gts import conform

    v = np.random.default_rng(2).choice(np.array([0, 1, 2, 4], dtype=np.int16), shape)
    src = _dev(v)
    for perm, signs in R.ORIENTATIONS:
        pl = _plan(shape, perm, signs)
        fwd = conform.conform_labels(src, pl)
        assert fwd.dtype == torch.int16 and np.array_equal(_host(fwd), R.reorient(v, perm, signs))
        back = conform.unconform_labels(fwd, pl)
        assert back.dtype == torch.int16 and np.array_equal(_host(back), v), (perm, signs)
        # the prediction kernels' layout, C-order [X, Y, Z]: same voxels, the gather absorbs the transpose
        zfast = torch.from_numpy(np.ascontiguousarray(_host(fwd))).to(DEV)
        assert np.array_equal(_host(conform.unconform_labels(zfast, pl, z_fastest=True)), v), (perm, signs)


def _check_trilinear(a, perm, signs, spacing):
    """|got - ref64| <= 1/2 ulp32(ref64) + 2^-45 vmax: three nested float64 lerps round a handful of times at
    2^-53 vmax (2^8 of margin, still 2^21 below float32 resolution), and the half ulp is the final rounding."""
    from gts import conform

    pl = _plan(a.shape[-3:], perm, signs, spacing)
    assert pl.resamples and pl.out_shape == R.conformed_shape(a.shape[-3:], perm, spacing)
    got = conform.conform_scan(_dev(a), pl)
    assert got.dtype == torch.float32 and tuple(got.shape) == (a.shape[0],) + pl.out_shape[::-1]
    ref, vmax = R.conform_trilinear(a, perm, signs, spacing)
    err = np.abs(_host(got).astype(np.float64) - ref)
    bound = 0.5 * R.ulp32(ref) + 2.0 ** -45 * vmax
    worst = float(np.max(err - bound))
    print(f"trilinear {a.dtype} {a.shape} {perm} {signs} {spacing}: max err {err.max():.3e}, max (err - bound) {worst:.3e}")
    assert np.all(err <= bound), (a.shape, perm, signs, spacing, float(err.max()))


@pytest.mark.parametrize("spacing", SPACINGS)
@pytest.mark.parametrize("shape", [(9, 8, 5), (40, 33, 6), (7, 1, 6)])
def test_trilinear(hip_lib, shape, spacing):
    for dtype in (np.int16, np.float32):
        a = _values(shape, dtype, 3)
        for perm, signs in MOVING:
            _check_trilinear(a, perm, signs, spacing)
        _check_trilinear(a, (0, 1, 2), (1, -1, 1), spacing)          # x stays the fastest axis: the row form


def test_trilinear_form_at_unit_spacing_returns_the_input(hip_lib):
    """Every t is 0: a + (b - a) * 0 is a, and the one rounding to float32 is exact."""
    from gts import conform

    for shape in [(9, 8, 5), (70, 37, 3)]:
        for dtype in (np.int16, np.float32):
            a = _values(shape, dtype, 4)
            src = _dev(a)
            for perm, signs in MOVING + [((0, 1, 2), (1, 1, 1))]:
                pl = _plan(shape, perm, signs)
                got = conform._gather(src, pl.source, pl.forward, conform.MODE_TRILINEAR, "test")
                want = R.reorient(a, perm, signs).astype(np.float32)
                assert got.dtype == torch.float32 and _host(got).tobytes() == want.tobytes()


@pytest.mark.parametrize("spacing", [(2, 2, 2), (0.5, 1, 0.5), (1.2, 1.2, 1.2), (1, 1, 2), (1.2, 1.5, 3)])
def test_nearest_forward_and_inverse(hip_lib, spacing):
    from gts import conform

    for shape in [(9, 8, 5), (40, 33, 6), (1, 7, 70)]:
        v = np.random.default_rng(5).choice(np.array([0, 1, 2, 4], dtype=np.int16), shape)
        for perm, signs in MOVING + [((0, 1, 2), (-1, -1, 1)), ((0, 1, 2), (1, -1, -1))]:
            pl = _plan(shape, perm, signs, spacing)
            if 2 in spacing:                         # t = 0.5 at every odd output index of that axis: takes idx1
                j = spacing.index(2)
                tb = pl.forward[perm[j]]
                assert np.all(tb.t[1::2] == 0.5) and np.all(tb.idx1[1::2] != tb.idx0[1::2])
            fwd = conform.conform_labels(_dev(v), pl)
            want = R.conform_nearest(v, perm, signs, spacing)
            assert tuple(fwd.shape) == pl.out_shape[::-1] and np.array_equal(_host(fwd), want), (shape, perm, spacing)
            back = conform.unconform_labels(fwd, pl)
            want_back = R.unconform_nearest(want, shape, perm, signs, spacing)
            assert tuple(back.shape) == tuple(shape)[::-1] and np.array_equal(_host(back), want_back)
            if min(spacing) >= 1:
                # |round(r s) / s - r| < 1/2: every voxel finds itself again.  That bound is for an index the inverse
                # table did not clamp; the last index of an axis (the first when it is reversed) is clamped when (n - 1) s has a fraction >= 1/2
                # (n_out - 1 = floor((n - 1) s) lies below its rounded position), and may then land on its neighbour.
                clamped = [np.floor((n - 1) * np.float64(sj) + 0.5) > np.floor((n - 1) * np.float64(sj))
                           for n, sj in zip(shape, spacing)]
                inner = tuple((slice(1, None) if f else slice(0, n - 1)) if c else slice(None)
                              for n, c, f in zip(shape, clamped, R.flips_of(perm, signs)))
                assert np.array_equal(want_back[inner], v[inner]), (shape, perm, spacing)


def test_device_tensor_goes_straight_into_the_intake(hip_lib):
    """prepare_scan on the device tensor equals prepare_scan on the host volumes."""
    from gts import intake, synth_mri

    img, _ = synth_mri.make_sample(3, (33, 30, 20))
    vols = [np.asfortranarray(img[..., c].astype(np.int16)) for c in range(4)]
    mean = np.array([0.4645, 0.6625, 0.4064, 0.3648], dtype=np.float32)
    std = np.array([0.1593, 0.1703, 0.1216, 0.1627], dtype=np.float32)
    want_img, want_crop, want_top = intake.prepare_scan(vols, mean, std)
    got_img, got_crop, got_top = intake.prepare_scan(intake.stage_scan(vols).to(DEV), mean, std)
    assert torch.equal(got_img, want_img) and got_top.tobytes() == want_top.tobytes()
    assert all(np.array_equal(a, b) for a, b in zip(got_crop, want_crop))


# ---- end to end: one child process writes the scans and runs segment_scans --conform on them ------------------

_E2E = r"""
import os, sys
import numpy as np, torch
from data_processing import nifti_io
from gts import synth_mri
from model.networks import init_graph_net
from utils.hyperparam_helpers import EvalParamSet
from scripts import segment_scans
from tests import conform_ref as R
tmp = sys.argv[1]
MODS = ("_flair.nii.gz", "_t1.nii.gz", "_t1ce.nii.gz", "_t2.nii.gz")
img, _ = synth_mri.make_sample(31, (64, 60, 40))
vols = [img[..., c].astype(np.int16) for c in range(4)]

def write(root, sid, volumes, affines):
    os.makedirs(os.path.join(root, sid), exist_ok=True)
    for v, ext, a in zip(volumes, MODS, affines):
        nifti_io.save_as_nifti(np.asfortranarray(v), os.path.join(root, sid, sid + ext), affine=a)

lps = np.array(nifti_io.BRATS_AFFINE, dtype=np.float64); lps[:3, 3] = (31.5, 29.5, -20.0)
ras = R.make_affine((0, 1, 2), (1, 1, 1), origin=(-31.5, -29.5, -20.0))
bp_perm, bp_signs = (2, 0, 1), (1, -1, 1)                  # stored (z, x, y): array axes run S, L, A (y reversed)
bp = R.make_affine(bp_perm, bp_signs, origin=(5.0, 6.0, 7.0))
half = lps.copy(); half[:3, 2] *= 2.0
raw = os.path.join(tmp, "raw")
write(raw, "A", vols, [lps] * 4)
write(raw, "B", [v[::-1, ::-1, :] for v in vols], [ras] * 4)
write(raw, "Bp", [R.unreorient(v, bp_perm, bp_signs) for v in vols], [bp] * 4)
write(raw, "C", [v[:, :, ::2] for v in vols], [half] * 4)
off = ras.copy(); off[0, 0] = 1.01
bad = os.path.join(tmp, "raw_bad")
write(bad, "A", vols, [lps] * 4)
write(bad, "D", [v[::-1, ::-1, :] for v in vols], [ras, ras, off, ras])
torch.manual_seed(0)
hp = EvalParamSet(in_feats=20, out_classes=4, layer_sizes=[256] * 4, gat_heads=None, gat_residuals=None)
gnn = os.path.join(tmp, "gnn.pt")
torch.save(init_graph_net("GSpool", hp).state_dict(), gnn)
rc1 = segment_scans.main(["-d", raw, "-o", os.path.join(tmp, "out"), "-g", gnn, "-n", "400", "--conform"])
rc2 = segment_scans.main(["-d", bad, "-o", os.path.join(tmp, "out_bad"), "-g", gnn, "-n", "400", "--conform",
                          "--min_component_voxels", "20"])
print("RC", rc1, rc2)
"""


@pytest.fixture(scope="module")
def e2e(tmp_path_factory, hip_lib):
    """(folder, the child's output): run once, read by the three tests below."""
    tmp = tmp_path_factory.mktemp("conform_e2e")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, REPO]))
    r = subprocess.run([sys.executable, "-c", _E2E, str(tmp)], cwd=PKG, env=env, capture_output=True, text=True,
                       timeout=500)
    assert r.returncode == 0 and "RC 0 1" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    return tmp, r.stdout


def _read(tmp, folder, sid):
    from data_processing import nifti_io

    fp = str(tmp / folder / f"{sid}.nii.gz")
    return nifti_io.read_nifti_raw(fp), nifti_io.read_affine(fp)[0]


def _input_affine(tmp, folder, sid):
    from data_processing import nifti_io

    return nifti_io.read_affine(str(tmp / folder / sid / f"{sid}_flair.nii.gz"))[0]


def test_e2e_equivariance(e2e):
    tmp, out = e2e
    a, a_aff = _read(tmp, "out", "A")
    assert a.dtype == np.int16 and a.shape == (64, 60, 40) and np.array_equal(a_aff, _input_affine(tmp, "raw", "A"))
    assert set(np.unique(a).tolist()) <= {0, 1, 2, 4} and (a != 0).any()
    b, b_aff = _read(tmp, "out", "B")
    assert b.shape == (64, 60, 40) and np.array_equal(b_aff, _input_affine(tmp, "raw", "B"))
    assert np.array_equal(b, a[::-1, ::-1, :])
    bp, bp_aff = _read(tmp, "out", "Bp")
    assert bp.shape == (40, 64, 60) and np.array_equal(bp_aff, _input_affine(tmp, "raw", "Bp"))
    assert np.array_equal(bp, R.unreorient(a, (2, 0, 1), (1, -1, 1)))
    lines = {ln.split(":")[0]: ln for ln in out.splitlines() if ": done" in ln}
    assert "conform: identity" in lines["A"]
    assert "conform: RAS -> LPS, spacing (1, 1, 1) mm, obliquity 0.0°" in lines["B"]
    assert "conform: SLA -> LPS" in lines["Bp"]


def test_e2e_resampled_scan(e2e):
    tmp, out = e2e
    c, c_aff = _read(tmp, "out", "C")
    assert c.dtype == np.int16 and c.shape == (64, 60, 20)
    assert np.array_equal(c_aff, _input_affine(tmp, "raw", "C")) and c_aff[2, 2] == 2.0
    assert set(np.unique(c).tolist()) <= {0, 1, 2, 4} and (c != 0).any()
    assert any("C: done" in ln and "spacing (1, 1, 2) mm" in ln for ln in out.splitlines())


def test_e2e_disagreeing_affines_are_skipped(e2e):
    tmp, out = e2e
    assert any(ln.startswith("D: skipped") and "disagree" in ln for ln in out.splitlines())
    assert os.path.exists(tmp / "out_bad" / "A.nii.gz") and not os.path.exists(tmp / "out_bad" / "D.nii.gz")
    assert any(ln.startswith("A: done") and "components" in ln and "conform: identity" in ln for ln in out.splitlines())
