"""Entropy maps restated in torch on the CPU in fp64 (the definitions of include/m355seg.h, uncertainty maps)."""
import math

import torch


def term(p):
    """p log p in fp64 with the zero rule: 0 for p <= 0, a NaN passes through"""
    p = p.double()
    return torch.where(p > 0, p * torch.log(p.clamp_min(1e-300)), torch.where(p != p, p, torch.zeros((), dtype=torch.float64)))


def entropy(p, kind='categorical'):
    """p [N, C, ...] (widened exactly to float32 first) -> fp64 [N, 1, ...], or [N, C, ...] for 'binary', where the
    definition's 1 - p is a float32 operation"""
    p = p.float()
    if kind == 'binary':
        return -(term(p) + term(1 - p))
    return -term(p).sum(dim=1, keepdim=True)


def tol_h(C):
    """2^-23 (C + (C - 1) ln max(C, 2)): a 1-ulp logf, the product and a float32 sum of C terms bounded by 1/e each"""
    return 2.0 ** -23 * (C + (C - 1) * math.log(max(C, 2)))


def ensemble_maps(members, kind='categorical'):
    """members: predictions in canonical orientation -> the four maps in fp64 (the mean formed in fp64)"""
    stacked = torch.stack([m.float() for m in members]).double()
    mean = stacked.mean(dim=0)
    if kind == 'binary':
        h = lambda p: -(term(p) + term(1 - p))
    else:
        h = lambda p: -term(p).sum(dim=1, keepdim=True)
    ent = h(mean)
    exp = torch.stack([h(m) for m in stacked]).mean(dim=0)
    return {'entropy': ent, 'expected_entropy': exp, 'mutual_information': (ent - exp).clamp_min(0),
            'confidence': mean.max(dim=1, keepdim=True).values}
