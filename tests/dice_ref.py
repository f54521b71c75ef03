"""Soft Dice over class regions + class-weighted cross-entropy in float64 torch on the CPU: the definition the
HIP kernels of csrc/gts_dice_ce.hip are held to.

Over the valid rows (0 <= y_i < C; a label of -100 is ignored, any other label makes the loss NaN), with
p_i = softmax(x_i) and m_rc the membership of class c in region r:

    q_ir = sum_c m_rc p_ic      t_ir = m_r,y_i
    I_r = sum_i q_ir t_ir       S_r = sum_i q_ir       T_r = sum_i t_ir
    dice_r = (2 I_r + smooth) / (S_r + T_r + smooth)   L_dice = 1 - mean_r dice_r
    CE = sum_i w[y_i] (lse_i - x_i,y_i) / sum_i w[y_i]
    L  = ce_weight CE + dice_weight L_dice             (a term of weight 0 is skipped and reads 0)
"""
from collections import namedtuple

import torch

IGNORE = -100
DiceRef = namedtuple("DiceRef", "loss ce l_dice dices grad grad_closed s_bound")


def region_sets(regions, n_classes):
    """Class-index lists of a named region set ("brats", "classes") or of explicit sets."""
    if regions == "brats":
        assert n_classes == 4
        return [[1, 2, 3], [2, 3], [3]]
    if regions == "classes":
        return [[c] for c in range(1, n_classes)]
    return [list(r) for r in regions]


def membership(regions, n_classes):
    m = torch.zeros(len(regions), n_classes, dtype=torch.float64)
    for r, members in enumerate(regions):
        m[r, members] = 1.0
    return m


def loss_terms(x, y, class_w, m, ce_weight, dice_weight, smooth):
    """(loss, CE, L_dice, dice_r, (I, S, T), sum of the row weights) through plain tensor ops; x float64 [N, C]."""
    n_classes = x.shape[1]
    valid = (y >= 0) & (y < n_classes)
    xv, yv = x[valid], y[valid]
    w = torch.ones(n_classes, dtype=torch.float64) if class_w is None else class_w.double()
    zero = x.sum() * 0.0
    ce, wsum = zero, w[yv].sum()
    if ce_weight != 0:
        nll = torch.logsumexp(xv, dim=1) - xv.gather(1, yv[:, None])[:, 0]
        ce = (w[yv] * nll).sum() / wsum
    l_dice, dices, ist = zero, torch.zeros(m.shape[0], dtype=torch.float64), None
    if dice_weight != 0:
        q = torch.softmax(xv, dim=1) @ m.T                      # [V, G]
        t = m.T[yv]                                             # [V, G]
        ist = ((q * t).sum(0), q.sum(0), t.sum(0))
        dices = (2.0 * ist[0] + smooth) / (ist[1] + ist[2] + smooth)
        l_dice = 1.0 - dices.mean()
    loss = zero
    if ce_weight != 0:
        loss = loss + ce_weight * ce
    if dice_weight != 0:
        loss = loss + dice_weight * l_dice
    return loss, ce, l_dice, dices, ist, wsum


def closed_form_grad(x, y, class_w, m, ce_weight, dice_weight, smooth, ist, wsum):
    """dL/dx from the formulas the gradient kernel implements (no autograd)."""
    n_classes, g = x.shape[1], m.shape[0]
    valid = (y >= 0) & (y < n_classes)
    yv = y[valid]
    p = torch.softmax(x[valid], dim=1)
    w = torch.ones(n_classes, dtype=torch.float64) if class_w is None else class_w.double()
    out = torch.zeros_like(p)
    if ce_weight != 0:
        onehot = torch.zeros_like(p).scatter_(1, yv[:, None], 1.0)
        out = out + ce_weight * w[yv][:, None] * (p - onehot) / wsum
    if dice_weight != 0:
        i_r, s_r, t_r = ist
        d = s_r + t_r + smooth
        a, b = -2.0 / (g * d), (2.0 * i_r + smooth) / (g * d * d)
        gic = (a[None, :] * m.T[yv] + b[None, :]) @ m           # [V, C]
        out = out + dice_weight * p * (gic - (gic * p).sum(1, keepdim=True))
    grad = torch.zeros_like(x)
    grad[valid] = out
    return grad


def dice_ce_ref(x, y, class_w=None, regions="brats", ce_weight=1.0, dice_weight=1.0, smooth=1.0):
    """The loss, its parts, its gradient by autograd and by the closed form, and S_bound = ce_weight max_c w_c / sum w
    + dice_weight sum_r (|a_r| + |b_r|), the largest possible |dL/dp|, for inputs of any float dtype."""
    x64 = x.detach().cpu().double().requires_grad_(True)
    y = y.detach().cpu()
    n_classes = x64.shape[1]
    nan = torch.tensor(float("nan"), dtype=torch.float64)
    m = membership(region_sets(regions, n_classes), n_classes)
    if bool(((y != IGNORE) & ((y < 0) | (y >= n_classes))).any()):
        return DiceRef(nan, nan, nan, nan.expand(m.shape[0]), None, None, float("nan"))
    cw = None if class_w is None else class_w.detach().cpu().double()
    loss, ce, l_dice, dices, ist, wsum = loss_terms(x64, y, cw, m, ce_weight, dice_weight, smooth)
    loss.backward()
    ist = None if ist is None else tuple(v.detach() for v in ist)
    wsum = wsum.detach()
    closed = closed_form_grad(x64.detach(), y, cw, m, ce_weight, dice_weight, smooth, ist, wsum)
    s_bound = 0.0
    if ce_weight != 0:
        s_bound += ce_weight * float((torch.ones(n_classes) if cw is None else cw).max() / wsum)
    if dice_weight != 0:
        d = ist[1] + ist[2] + smooth
        g = m.shape[0]
        s_bound += dice_weight * float(((2.0 / (g * d)).abs() + ((2.0 * ist[0] + smooth) / (g * d * d)).abs()).sum())
    return DiceRef(loss.detach(), ce.detach(), l_dice.detach(), dices.detach(), x64.grad, closed, s_bound)
