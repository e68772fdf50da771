"""Uncertainty maps on the device (csrc/uncertainty.hip): ops.predictive_entropy and the ensembles' reducer
with the entropy accumulator against fp64 torch on the CPU (uncertainty_ref), and the bit-for-bit relations between
the three entry points."""
import itertools
import math

import pytest
import torch
from torch import nn

import uncertainty_ref as uref
from segmentation_pipeline_amd import ops
from segmentation_pipeline_amd.models import EnsembleFlips, EnsembleModels, EnsembleOrientations, ModularUNet
from segmentation_pipeline_amd.models import ensemble as E

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SIZES = [(5, 7, 9), (17, 33, 31), (4, 6, 8), (16, 16, 16)]     # odd: element loads; multiples of 8: 16-byte loads
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
CASES = [(1, 'binary'), (2, 'categorical'), (4, 'categorical'), (4, 'binary'), (64, 'categorical')]
WORST = {}


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def note(key, err, tol):
    WORST[key] = max(WORST.get(key, 0.0), float(err) / tol)


def probabilities(g, N, C, size, kind):
    z = 2.5 * torch.randn((N, C) + size, generator=g)
    return torch.sigmoid(z) if kind == 'binary' else torch.softmax(z, dim=1)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[1])
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"C{c[0]}-{c[1]}")
def test_predictive_entropy_against_fp64(case, dtype):
    """every size in turn; exact zeros and ones planted (the entropy there is exactly 0, not NaN), a NaN planted (NaN at
    that voxel only); the confidence is the maximum channel value"""
    C, kind = case
    g = torch.Generator().manual_seed(17 * C + len(kind) + len(str(dtype)))
    tol = uref.tol_h(C)
    for size in SIZES:
        p = probabilities(g, 2, C, size, kind).to(dtype)
        flat = p.view(2, C, -1)
        flat[:, :, 1] = 0.0
        flat[:, 0, 1] = 1.0                     # a one-hot voxel: zeros and a one
        flat[:, :, 2] = 0.0                     # all zeros
        flat[1, C - 1, 4] = float("nan")
        h, conf = ops.predictive_entropy(p.to(DEV), kind, confidence=True)
        K = C if kind == 'binary' else 1
        assert h.shape == (2, K) + size and conf.shape == (2, 1) + size and h.dtype == conf.dtype == torch.float32
        h, conf = h.cpu(), conf.cpu()
        want = uref.entropy(p, kind)
        nan = want.isnan()
        assert torch.equal(h.isnan(), nan) and int(nan.sum()) == 1
        err = (h.double() - want)[~nan].abs().max().item()
        note(f"predictive_entropy C={C} {kind}", err, tol)
        print(f"C={C} {kind} {dtype} {size}: max error {err:.3e}, tol {tol:.3e}")
        assert err <= tol
        hv = h.view(2, K, -1)
        assert (hv[:, :, 1] == 0).all() and (hv[:, :, 2] == 0).all() and not hv[:, :, 1].isnan().any()
        wc = p.float().max(dim=1, keepdim=True).values
        assert torch.equal(conf.isnan(), wc.isnan()) and torch.equal(conf[~wc.isnan()], wc[~wc.isnan()])
        assert same_bits(ops.predictive_entropy(p.to(DEV), kind).cpu(), h)          # without the confidence, and again


def _reduce(members, transforms, size, kind, dirty=False):
    """the reducer on member predictions given in the members' own orientation -> (mean, maps)"""
    N, C = members[0].shape[:2]
    red = E._Reducer('mean', (N, C) + size, DEV, kind)
    if dirty:
        red.acc = torch.full((N, C) + size, float("nan"), device=DEV)
        red.eacc = torch.full(red._entropy_shape(), float("nan"), device=DEV)
    for m, (perm, fm) in zip(members, transforms):
        red.add(m.to(DEV), perm, fm)
    mean, _ = red.result()
    return mean, red.uncertainty()


@pytest.mark.parametrize("kind", ["categorical", "binary"])
@pytest.mark.parametrize("members", [3, 8])
def test_reducer_with_the_entropy_accumulator(members, kind):
    """all six permutations and all eight flip masks over the calls, size (5, 6, 7): random member predictions in the
    member's orientation against _torch_back + the fp64 formulas.  All extents differ: a wrong permutation cannot pass"""
    size, C, N = (5, 6, 7), 3, 2
    g = torch.Generator().manual_seed(members)
    perms = list(itertools.permutations(range(3)))
    every = [(perm, fm) for perm in perms for fm in range(8)]
    tol = 2 * uref.tol_h(C) + members * 2.0 ** -23 * (1 + math.log(C))
    worst = 0.0
    for start in range(0, len(every), members):
        transforms = every[start:start + members]
        transforms += every[:members - len(transforms)]
        preds = [probabilities(g, N, C, tuple(size[p] for p in perm), kind) for perm, _ in transforms]
        mean, maps = _reduce(preds, transforms, size, kind)
        back = [E._torch_back(p, perm, fm) for p, (perm, fm) in zip(preds, transforms)]
        want = uref.ensemble_maps(back, kind)
        K = C if kind == 'binary' else 1
        for k in E.UNCERTAINTY_MAPS:
            got = maps[k].cpu()
            assert got.shape == (N, 1 if k == 'confidence' else K) + size
            err = (got.double() - want[k]).abs().max().item()
            worst = max(worst, err)
            assert err <= tol, (k, transforms, err, tol)
        assert (maps['mutual_information'] >= 0).all()
        assert same_bits(maps['entropy'], ops.predictive_entropy(mean, kind))
    note(f"reducer E={members} {kind}", worst, tol)
    print(f"E={members} {kind}: max error {worst:.3e}, tol {tol:.3e}")


@pytest.mark.parametrize("kind", ["categorical", "binary"])
def test_bit_for_bit_relations(kind):
    size, C, N = (5, 6, 7), 3, 2
    g = torch.Generator().manual_seed(2)
    p = probabilities(g, N, C, size, kind)
    ident = ((0, 1, 2), 0)
    # the same prediction four times: no disagreement at all, and the entropy is the prediction's own
    mean, maps = _reduce([p] * 4, [ident] * 4, size, kind)
    assert (maps['mutual_information'] == 0).all() and same_bits(mean.cpu(), p)
    assert same_bits(maps['entropy'], ops.predictive_entropy(p.to(DEV), kind))
    assert same_bits(maps['expected_entropy'], maps['entropy'])
    # accumulators that held NaNs give the bits of clean ones (first != 0 initialises); a call twice gives the same bits
    transforms = [((2, 0, 1), 5), ((1, 0, 2), 2), ((0, 1, 2), 7)]
    preds = [probabilities(g, N, C, tuple(size[q] for q in perm), kind) for perm, _ in transforms]
    mean_a, a = _reduce(preds, transforms, size, kind)
    mean_b, b = _reduce(preds, transforms, size, kind, dirty=True)
    mean_c, c = _reduce(preds, transforms, size, kind)
    assert same_bits(mean_a, mean_b) and same_bits(mean_a, mean_c)
    for k in E.UNCERTAINTY_MAPS:
        assert same_bits(a[k], b[k]) and same_bits(a[k], c[k]), k
    # the mean does not depend on whether the entropy accumulator runs beside it
    plain = E._Reducer('mean', (N, C) + size, DEV)
    for m, (perm, fm) in zip(preds, transforms):
        plain.add(m.to(DEV), perm, fm)
    assert plain.eacc is None and same_bits(plain.result()[0], mean_a)
    # a NaN in one member stays a NaN in its voxel's maps, and only there
    bad = [q.clone() for q in preds]
    bad[1].view(-1)[11] = float("nan")
    _, d = _reduce(bad, transforms, size, kind)
    assert int(d['mutual_information'].isnan().sum()) == 1 and int(d['entropy'].isnan().sum()) == 1


def _small_unet(sigmoid=False):
    torch.manual_seed(0)
    extra = dict(hypothesis_class=nn.Sigmoid, hypothesis_params={}) if sigmoid else {}
    return ModularUNet(2, 3, [8, 16], 2, **extra).to(DEV).eval()


@pytest.mark.parametrize("which", ["flips", "orientations", "models", "flips-binary"])
def test_ensembles_fill_last_uncertainty(which):
    binary = which.endswith("binary")
    kind = 'binary' if binary else 'categorical'
    model = _small_unet(binary)
    size = (16, 16, 16)
    x = torch.randn((1, 2) + size, generator=torch.Generator().manual_seed(1)).to(DEV)
    make = {"flips": lambda **kw: EnsembleFlips(model, **kw), "flips-binary": lambda **kw: EnsembleFlips(model, **kw),
            "orientations": lambda **kw: EnsembleOrientations(model, **kw),
            "models": lambda **kw: EnsembleModels([model, _small_unet(), model], **kw)}[which]
    torch.manual_seed(0)
    with torch.no_grad():
        plain = make()
        before = plain(x)
        ens = make(uncertainty=True, uncertainty_kind=kind)
        out = ens(x)
    assert plain.last_uncertainty is None and ens.last_votes is None
    assert same_bits(out, before)                                   # the prediction's bits as before
    u = ens.last_uncertainty
    assert tuple(u) == E.UNCERTAINTY_MAPS
    for k in E.UNCERTAINTY_MAPS:
        assert u[k].shape == (1, 3 if binary and k != 'confidence' else 1) + size and u[k].isfinite().all(), k
    assert (u['mutual_information'] >= 0).all() and (u['entropy'] >= 0).all()
    if which != "models":
        assert u['mutual_information'].max() > 0                    # flipped members do disagree somewhere
    assert same_bits(u['entropy'], ops.predictive_entropy(out, kind))
    assert same_bits(u['confidence'], out.max(dim=1, keepdim=True).values)


def test_zz_report_worst_errors():
    """(not a check of its own: prints the largest errors the tests above saw, in units of their tolerance)"""
    for k, v in sorted(WORST.items()):
        print(f"{k}: largest error / tolerance = {v:.3f}")
    assert all(v <= 1 for v in WORST.values())
