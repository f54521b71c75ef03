"""Joint GNN + CNN training step (model/joint_model.py) on one BraTS-size synthetic sample, against its parts.

    python tools/measure_joint_training.py --out profiles/joint/measure.json [--reps 20] [--skip-torch]

One sample: gts.synth_mri scan -> brain crop -> standardized image -> gts.graphgen.build_graph (15 000
supervoxels asked for, k = 10).  Networks: GSpool [256]*4 and the 8 -> 16 -> 4 refinement CNN, freshly
initialised.  Two crops: the one the GNN's own prediction selects, and a fixed 96^3 box (the shape of
profiles/cnn/).  Per crop, HIP events, median of --reps after two warm-ups, all in this process:
  * JointModel.train_step;
  * GNN.train_step on the same graph and RefinementModel.train_step on the same crop (the two separate steps
    the joint one replaces), and their sum;
  * the three launches the joint step adds: J1 (with K16 as its sibling), conv1's data gradient on the
    logit channels, J2; J1 / K16 / J2 also as a fraction of the 8 TB/s HBM peak over their compulsory bytes
    (J1, K16: 4 (Ci + Ct) + 4 Ci + 2 = 50 B per crop voxel; J2: 4 Ct B per crop voxel + 4 B per listed voxel +
    4 Ct B per node; the widths come from the networks); the conv1 launch includes the copy of the weight slice;
  * unless --skip-torch, at the 96^3 box only: the same step with the glue and the CNN written in plain torch
    (advanced indexing, autograd's index_put backward, MIOpen convolutions with cudnn.benchmark = True, two
    torch.optim.AdamW); the graph network is the same module on both sides.
--profile-workload runs five joint steps at the 96^3 box and nothing else (for rocprofv3 --kernel-trace).
"""
import argparse
import io
import json
import os
import sys
from contextlib import redirect_stdout

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "gnn-tumor-seg_amd")]

from gts import build, conv3d, graphgen, ops, synth_mri  # noqa: E402

HBM_PEAK = 8.0e12


def timed(fn, reps):
    """Median milliseconds of `fn` over `reps` event-bracketed runs after two warm-ups."""
    for _ in range(2):
        fn()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def make_sample(seed, n_nodes, dev):
    from data_processing.image_processing import determine_brain_crop, normalize_img, standardize_img
    from scripts.preprocess_dataset import STANDARDIZATION_STATS, swap_labels_from_brats

    img, lab = synth_mri.make_sample(seed)
    crop = determine_brain_crop(img)
    data = standardize_img(normalize_img(img[crop]), np.float32(STANDARDIZATION_STATS[0]),
                           np.float32(STANDARDIZATION_STATS[1])).astype(np.float32)
    labels = swap_labels_from_brats(lab[crop])
    res = graphgen.build_graph(data, labels, n_nodes, 0.5, 10)
    graph = graphgen.graph_from_edges(res["edges"], res["feats"].shape[0])
    lists = ops.SupervoxelLists(np.ascontiguousarray(res["partition"]), graph.n, dev)
    return {
        "graph": graph.to(dev),
        "feats": torch.from_numpy(np.asarray(res["feats"], dtype=np.float32)).to(dev),
        "node_labels": torch.from_numpy(np.asarray(res["labels"]).astype(np.int64)).to(dev),
        "img": torch.from_numpy(np.ascontiguousarray(data)).to(dev),
        "svs": lists.svs,
        "voxel_labels": torch.from_numpy(np.ascontiguousarray(labels).astype(np.int64)).to(dev),
        "lists": lists,
    }


def centred_box(shape, edge, dev):
    idx = [np.arange(max(0, (n - edge) // 2), max(0, (n - edge) // 2) + min(edge, n)) for n in shape]
    return ops.CropBox(*idx, shape, dev)


def measure_crop(name, box, s, hps, reps, dev, with_torch):
    from model.cnn_model import RefinementModel
    from model.gnn_model import GNN
    from model.joint_model import JointModel

    gnn_hp, cnn_hp = hps
    torch.manual_seed(0)
    with redirect_stdout(io.StringIO()):
        joint = JointModel("GSpool", gnn_hp, cnn_hp, None)
        gnn = GNN("GSpool", gnn_hp, None)
        cnn = RefinementModel(cnn_hp, None, None)
    joint.crop_box = lambda logits, svs: box
    v = int(np.prod(box.shape))
    n = s["graph"].n
    out = {"crop": name, "box": list(box.shape), "voxels": v, "nodes": n, "listed_voxels": int(s["lists"].list_ptr[-1])}
    args = (s["graph"], s["feats"], s["node_labels"], s["img"], s["svs"], s["voxel_labels"], s["lists"])
    out["joint_step_ms"] = timed(lambda: joint.train_step(*args), reps)
    out["gnn_step_ms"] = timed(lambda: gnn.train_step(s["graph"], s["feats"], s["node_labels"]), reps)
    with torch.no_grad():
        table = joint.graph_net(s["graph"], s["feats"]).contiguous()
    x = ops.crop_concat_rows(s["img"], s["svs"], table, joint.bg_row, box)
    y = joint.cropped_labels(s["voxel_labels"], box)
    out["cnn_step_ms"] = timed(lambda: cnn.train_step(x, y), reps)
    out["sum_of_parts_ms"] = out["gnn_step_ms"] + out["cnn_step_ms"]
    w1 = joint.conv_net.conv_layers[0].weight.detach()
    ct = table.shape[1]                      # node-logit width; the image has the network's other input channels
    ci = cnn_hp.in_feats - ct
    row_bytes = 4 * (ci + ct) + 4 * ci + 2         # J1 / K16 per crop voxel: the output row, the image row, the int16 id
    dz1 = torch.randn(v, w1.shape[0], device=dev)
    dxl = torch.randn(v, ct, device=dev)
    launches = {
        "J1 crop_concat_rows": (lambda: ops.crop_concat_rows(s["img"], s["svs"], table, joint.bg_row, box), row_bytes * v),
        "K16 crop_concat (sibling)": (lambda: ops.crop_concat(s["img"], s["svs"], table, joint.bg_row, box), row_bytes * v),
        "conv1 data gradient, logit channels": (lambda: conv3d.conv3d_bwd_data(dz1, w1[:, ci:].contiguous(), box.shape), None),
        "J2 crop_concat_rows_bwd": (lambda: ops.crop_concat_rows_bwd(dxl, s["lists"], box, 0),
                                    4 * ct * v + 4 * out["listed_voxels"] + 4 * ct * n),
    }
    out["launches"] = {}
    for label, (fn, nbytes) in launches.items():
        ms = timed(fn, reps)
        row = {"ms": ms}
        if nbytes is not None:
            row.update(compulsory_bytes=nbytes, tb_per_s=nbytes / ms / 1e9, hbm_peak_fraction=nbytes / (ms * 1e-3) / HBM_PEAK)
        out["launches"][label] = row
    out["new_launches_ms"] = sum(out["launches"][k]["ms"] for k in out["launches"] if not k.startswith("K16"))
    if with_torch:
        out["torch_glue_step_ms"] = timed(torch_step(joint, s, box, gnn_hp, cnn_hp), max(3, reps // 4))
    return out


def torch_step(joint, s, box, gnn_hp, cnn_hp):
    """The step with the glue and the CNN in plain torch on the same GPU; same graph network module."""
    from model.networks import CnnRefinementNet, init_graph_net

    dev = s["img"].device
    gnet = init_graph_net("GSpool", gnn_hp).to(dev)
    cnet = CnnRefinementNet(cnn_hp.in_feats, cnn_hp.out_classes, cnn_hp.layer_sizes).to(dev)
    opts = [torch.optim.AdamW(gnet.parameters(), lr=gnn_hp.lr, weight_decay=gnn_hp.w_decay),
            torch.optim.AdamW(cnet.parameters(), lr=cnn_hp.lr, weight_decay=cnn_hp.w_decay)]
    xs, ys, zs = (d.long() for d in box.dev)
    ids = s["svs"].long()
    rows = torch.where(ids < 0, ids + s["graph"].n + 1, ids)
    y = joint.cropped_labels(s["voxel_labels"], box).view(1, *box.shape)
    w_cnn, w_gnn, bg = joint.cnn_class_weights, joint.gnn_class_weights, joint.bg_row.view(1, -1)

    def step():
        node_logits = gnet(s["graph"], s["feats"])
        voxel = torch.cat([node_logits, bg], dim=0)[rows]
        x = torch.cat([s["img"], voxel], dim=-1)[xs[:, None, None], ys[None, :, None], zs[None, None, :]]
        out = cnet(x.movedim(-1, 0)[None])
        loss = F.cross_entropy(out, y, weight=w_cnn) + F.cross_entropy(node_logits, s["node_labels"], weight=w_gnn)
        for o in opts:
            o.zero_grad()
        loss.backward()
        for o in opts:
            o.step()

    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--nodes", type=int, default=15000, help="supervoxels asked of SLIC (preprocess_dataset's default)")
    ap.add_argument("--skip-torch", action="store_true")
    ap.add_argument("--profile-workload", action="store_true")
    args = ap.parse_args()
    build.build()
    from utils.hyperparam_helpers import populate_hardcoded_hyperparameters

    if not torch.cuda.is_available():
        raise SystemExit("measure_joint_training needs an MI355X: there is nothing to measure on a CPU")
    dev = torch.device("cuda", 0)
    torch.backends.cudnn.benchmark = True
    with redirect_stdout(io.StringIO()):
        hps = (populate_hardcoded_hyperparameters("GSpool"), populate_hardcoded_hyperparameters("CNN"))
    s = make_sample(21, args.nodes, dev)
    fixed = centred_box(tuple(s["svs"].shape), 96, dev)
    if args.profile_workload:
        from model.joint_model import JointModel

        with redirect_stdout(io.StringIO()):
            joint = JointModel("GSpool", *hps, None)
        joint.crop_box = lambda logits, svs: fixed
        for _ in range(5):
            joint.train_step(s["graph"], s["feats"], s["node_labels"], s["img"], s["svs"], s["voxel_labels"], s["lists"])
        torch.cuda.synchronize()
        return
    from model.joint_model import JointModel

    with redirect_stdout(io.StringIO()):
        probe = JointModel("GSpool", *hps, None)
        with torch.no_grad():
            own = probe.crop_box(probe.graph_net(s["graph"], s["feats"]), s["svs"])
    del probe
    results = []
    for name, box, with_torch in (("fixed 96^3", fixed, not args.skip_torch), ("the GNN's own crop", own, False)):
        r = measure_crop(name, box, s, hps, args.reps, dev, with_torch)
        results.append(r)
        print(json.dumps({k: v for k, v in r.items() if k != "launches"}))
        for label, row in r["launches"].items():
            print(f"    {label:40s} {row['ms']:8.3f} ms" + (f"  {row['hbm_peak_fraction']:.3f} of the HBM peak"
                                                            if "hbm_peak_fraction" in row else ""))
        torch.cuda.empty_cache()
        if args.out:      # rewritten after every crop
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump({"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "reps": args.reps,
                           "volume": list(s["svs"].shape), "results": results}, f, indent=1)


if __name__ == "__main__":
    main()
