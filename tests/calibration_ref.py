"""Calibration tables and sums restated in torch on the CPU (the definitions of include/m355seg.h, m355_eval_calibration):
tables by boolean masks with the float32 bin rule, the fixed point as torch.round(q.double() * 2**32), sums in fp64."""
import torch

FIX = 2 ** 32
EPS = 1e-8


def bin_index(q, bins):
    """min((int)(q * (float)bins), bins - 1) of float32 confidences in [0, 1]: one float32 multiply and a truncation"""
    q = q.float()
    return torch.clamp((q * torch.tensor(float(bins), dtype=torch.float32)).to(torch.int64), max=bins - 1)


def table(valid, q, hit, bins):
    """int [bins][3]: count, hits and the fixed-point confidence sum of the valid entries"""
    q = torch.where(valid, q.float(), torch.zeros(()))     # (invalid values must not reach the integer cast)
    b = bin_index(q, bins)
    fixed = torch.round(q.double() * FIX)
    out = []
    for k in range(bins):
        m = valid & (b == k)
        out.append([int(m.sum()), int((m & hit).sum()), int(fixed[m].sum().item())])
    return out


def safe(p):
    return (p + EPS) / (1 + EPS)


def reference(scores, target, bins, kind):
    """scores [C, *spatial] (any float type, widened exactly); target of the same shape (one-hot / soft: positive where
    != 0, the class is torch.argmax) or one channel index per voxel.  -> dict: top [B][3] (categorical), classwise
    [C][B][3], invalid (int, or a list per channel for 'binary'), brier, nll (fp64 sums), terms = (brier terms, nll
    terms), valid (voxels, or pairs for 'binary')"""
    C = scores.shape[0]
    p = scores.reshape(C, -1).float()
    S = p.shape[1]
    if tuple(target.shape) == tuple(scores.shape):
        t = target.reshape(C, -1)
        pos = t != 0
        tcls = torch.argmax(t.double(), dim=0)
        tok = torch.ones(S, dtype=torch.bool)
    else:
        idx = target.reshape(-1).long()
        tok = (idx >= 0) & (idx < C)
        tcls = torch.where(tok, idx, torch.zeros_like(idx))
        pos = (torch.arange(C)[:, None] == idx[None]) & tok[None]
    inr = (p >= 0) & (p <= 1)
    y = pos.double()
    sq = (torch.where(inr, p, torch.zeros(())).double() - y) ** 2
    out = {}
    if kind == 'categorical':
        valid = inr.all(dim=0) & tok
        pv = torch.where(valid[None], p, torch.zeros(()))
        arg = torch.argmax(pv, dim=0)
        q = pv.gather(0, arg[None])[0]
        out['top'] = table(valid, q, arg == tcls, bins)
        out['classwise'] = [table(valid, pv[c], pos[c], bins) for c in range(C)]
        out['invalid'] = int(S - valid.sum())
        out['brier'] = sq[:, valid].sum().item()
        pt = pv.gather(0, tcls[None])[0].double()
        out['nll'] = (-torch.log(safe(pt)))[valid].sum().item()
        nv = int(valid.sum())
        out['terms'] = (C * nv, nv)
        out['valid'] = nv
    else:
        valid = inr & tok[None]
        pv = torch.where(valid, p, torch.zeros(())).double()
        out['classwise'] = [table(valid[c], p[c], pos[c], bins) for c in range(C)]
        out['invalid'] = [int(S - valid[c].sum()) for c in range(C)]
        out['brier'] = sq[valid].sum().item()
        out['nll'] = (-torch.where(pos, torch.log(safe(pv)), torch.log(safe(1.0 - pv))))[valid].sum().item()
        nv = int(valid.sum())
        out['terms'] = (nv, nv)
        out['valid'] = nv
    return out


def table_stats(tab):
    """(ece, mce, confidence, accuracy) of an int table [B][3], Python fp64 from the integers; NaN when it is empty"""
    n = sum(r[0] for r in tab)
    if n == 0:
        return (float('nan'),) * 4
    gaps = [(c, abs(h / c - f / FIX / c)) for c, h, f in tab if c]
    return (sum(c / n * g for c, g in gaps), max(g for _, g in gaps), sum(r[2] for r in tab) / FIX / n,
            sum(r[1] for r in tab) / n)
