"""TEST INFRASTRUCTURE ONLY: the definition of the ensemble prediction in numpy / torch-CPU float64,
with the mirrors applied to the DATA (flip, net, flip back), so that the product's weight-mirroring identity is
tested and not assumed.

    P    = mean over members of softmax(node logits)                              [N, C]
    box  = the dilated box around the voxels whose node's arg-max of P is not 0   (oracle.joint_ref)
    y_mv = unflip_v(cnn_m(flip_v(cat([img, table_m[svs]], -1)[box])))             member-major, view-minor
    Q    = mean over all (m, v) of softmax(y_mv)                                  [cx, cy, cz, C]
    label = first-maximum arg-max of Q inside the box, 0 outside
"""
import numpy as np
import torch

from oracle import joint_ref


def softmax64(logits):
    x = np.asarray(logits, dtype=np.float64)
    e = np.exp(x - x.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def mean_softmax(logit_sets):
    """Mean over the sets (in order) of their row softmax, float64."""
    total = np.zeros(np.asarray(logit_sets[0]).shape, dtype=np.float64)
    for s in logit_sets:
        total += softmax64(s)
    return total / len(logit_sets)


def top_two_margin(probs):
    """Largest minus second largest entry along the last axis (0 for a single class)."""
    p = np.sort(np.asarray(probs, dtype=np.float64), axis=-1)
    return p[..., -1] - p[..., -2] if p.shape[-1] > 1 else np.zeros(p.shape[:-1])


def as_float64_cnn(net):
    """A float64 CPU copy of a two-layer refinement CNN (any module with conv_layers.{0,1})."""
    c1, c2 = net.conv_layers
    ref = joint_ref.RefCnnRefinementNet(c1.in_channels, c2.out_channels, [c1.out_channels]).double()
    ref.load_state_dict({k: v.detach().cpu().double() for k, v in net.state_dict().items()})
    return ref.eval()


def mirrored_view_logits(net64, x, flips):
    """unmirror(net(mirror(x))) for channels-last x [cx, cy, cz, Cin] (float64 tensor) -> [cx, cy, cz, Cout]."""
    dims = [a for a in range(3) if flips[a]]
    xin = torch.flip(x, dims) if dims else x
    with torch.no_grad():
        y = net64(xin.movedim(-1, 0).unsqueeze(0))[0].movedim(0, -1)
    return torch.flip(y, dims) if dims else y


def node_prediction(node_logit_sets, svs):
    """(P [N, C], label volume of the arg-max of P with 0 on the background, margin volume of P's top two)."""
    probs = mean_softmax(node_logit_sets)
    ids = np.asarray(svs).astype(np.int64)
    labels = np.append(probs.argmax(axis=1), 0)[ids].astype(np.int16)
    margin = np.append(top_two_margin(probs), np.inf)[ids]
    return probs, labels, margin


def ensemble_ref(node_logit_sets, cnns, views, img, svs, background_logits):
    """node_logit_sets: the members' node logits [N, C]; cnns: their CNNs (float64 copies are made); views: flip
    triples; img [X, Y, Z, Ci]; svs [X, Y, Z] int16; background_logits [[C floats]].
    Returns dict(node_probs, crop (np.ix_), probs [cx, cy, cz, C], margin [cx, cy, cz], labels int16 like svs)."""
    node_probs, gnn_labels, _ = node_prediction(node_logit_sets, svs)
    crop = joint_ref.determine_tumor_crop_ref(gnn_labels)
    ids = np.asarray(svs).astype(np.int64)
    img64 = torch.from_numpy(np.asarray(img, dtype=np.float64))
    total, terms = None, 0
    for table, net in zip(node_logit_sets, cnns):
        rows = np.concatenate([np.asarray(table, dtype=np.float64), np.asarray(background_logits, dtype=np.float64)])
        x = torch.cat([img64, torch.from_numpy(rows[ids])], dim=-1)[crop]
        net64 = as_float64_cnn(net)
        for flips in views:
            p = softmax64(mirrored_view_logits(net64, x, flips).numpy())
            total = p if total is None else total + p
            terms += 1
    probs = total / terms
    labels = np.zeros(ids.shape, dtype=np.int16)
    labels[crop] = probs.argmax(axis=-1)
    return dict(node_probs=node_probs, crop=crop, probs=probs, margin=top_two_margin(probs), labels=labels)
