"""ops.CONV_PROFILE, the list bench.py builds its roofline from: which records the convolutions of each activation flow
append -- (tag, flops, start event, end event, plan, algorithmic bytes), launch for launch and in launch order -- and the
three gates (CONV_PROFILE is None, CONV_PROFILE_KEYS, CONV_PROFILE_EVERY).  Every expected value is computed here:
flops = 2 k^3 Cin Cout N voxels_out, bytes = input once + output once + fp32 weights once at the element sizes the flow
reports, plan = ops.conv_plan of a descriptor built here (None for the weight gradient of the two 16-bit flows)."""
import ctypes as C

import pytest
import torch

from segmentation_pipeline_amd import _lib, ops

pytestmark = pytest.mark.gpu

D = 8                      # 8^3 voxels: one tile of every plan, the smallest volume all flows accept
S = D * D * D
FWD, BWW, BWD = "conv3d_fwd", "conv3d_bwd_weight", "conv3d_bwd_data"


def rnd(*shape, seed=0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).cuda()


def flops(N, Cin, Cout):
    return 2.0 * 27 * Cin * Cout * N * S


def nbytes(N, Cin, Cout, in_elem, out_elem):
    """input once + output once + the fp32 filter once"""
    return float(N) * S * (Cin * in_elem + Cout * out_elem) + 4.0 * Cin * Cout * 27


def desc(N, Cin, Cout, mode, xbs=0, ybs=0):
    return ops._conv_desc(N, Cin, Cout, D, D, D, 3, 1, 1, xbs, ybs, compute=ops._COMPUTE[mode])


def params(Cin, Cout, grad=True, seed=0):
    w = (rnd(Cout, Cin, 3, 3, 3, seed=seed) * 0.1).requires_grad_(grad)
    b = (rnd(Cout, seed=seed + 1) * 0.1).requires_grad_(grad)
    return w, b


class profiled:
    """`with profiled(mode) as prof:` -- ops.CONV_PROFILE = prof = [] in precision `mode`; every global is put back"""

    def __init__(self, mode, keys=None, every=1, prof=True):
        self.mode, self.keys, self.every, self.prof = mode, keys, every, [] if prof else None

    def __enter__(self):
        self.saved = (ops.CONV_PROFILE, ops.CONV_PROFILE_KEYS, ops.CONV_PROFILE_EVERY, ops._prof_seen, ops.get_precision())
        ops.set_precision(self.mode)
        ops.CONV_PROFILE, ops.CONV_PROFILE_KEYS, ops.CONV_PROFILE_EVERY, ops._prof_seen = self.prof, self.keys, self.every, 0
        return self.prof

    def __exit__(self, *exc):
        ops.CONV_PROFILE, ops.CONV_PROFILE_KEYS, ops.CONV_PROFILE_EVERY, ops._prof_seen, mode = self.saved
        ops.set_precision(mode)


def check_records(prof, expected):
    """prof against [(tag, flops, plan, bytes)], in order; both events of every record were recorded"""
    torch.cuda.synchronize()
    got = [(r[0], r[1], r[4], r[5]) for r in prof]
    for g, e in zip(got, expected):
        print("conv_profile", g, "expected", e)
    assert [g[0] for g in got] == [e[0] for e in expected]
    assert got == expected
    for r in prof:
        assert len(r) == 6
        assert r[2].elapsed_time(r[3]) >= 0.0


def tensor_flow_expected(N, Cin, Cout, mode, bww_plan=True):
    """forward + backward of ops.conv3d on dense fp32 tensors: 4-byte elements on both sides in every mode"""
    d = desc(N, Cin, Cout, mode, Cin * S, Cout * S)
    dd = desc(N, Cin, Cout, mode, 0, Cout * S)
    f, b = flops(N, Cin, Cout), nbytes(N, Cin, Cout, 4, 4)
    return [(FWD, f, ops.conv_plan(d, 0), b), (BWW, f, ops.conv_plan(d, 2) if bww_plan else None, b),
            (BWD, f, ops.conv_plan(dd, 1), b)]


# ----------------------------------------------------------------------------------------------- fp32 tensor flow
@pytest.mark.parametrize("Cin,Cout,softmax", [(8, 8, False), (2, 8, False), (8, 3, True)],
                         ids=["8to8", "edge_cin2", "out_conv_softmax"])
def test_fp32_tensor_flow(Cin, Cout, softmax):
    N = 2
    x = rnd(N, Cin, D, D, D, seed=3).requires_grad_(True)
    w, b = params(Cin, Cout)
    with profiled("fp32") as prof:
        ops.conv3d(x, w, b, softmax=softmax).sum().backward()
    check_records(prof, tensor_flow_expected(N, Cin, Cout, "fp32"))
    assert x.grad is not None and w.grad is not None and b.grad is not None


def test_bf16_twin_flow(monkeypatch):
    """fp32 tensors between the layers, c8 operands inside the autograd function: the records keep 4-byte elements and the
    weight gradient has no plan"""
    monkeypatch.setattr(ops, "H16_TRAIN_C8ONLY", False)
    N = 2
    x = rnd(N, 8, D, D, D, seed=3).requires_grad_(True)
    w, b = params(8, 8)
    with profiled("bf16") as prof:
        ops.conv3d(x, w, b).sum().backward()
    check_records(prof, tensor_flow_expected(N, 8, 8, "bf16", bww_plan=False))
    assert x.grad is not None and w.grad is not None


# ------------------------------------------------------------------------------------------------------- c8 flows
@pytest.mark.parametrize("mode", ["bf16", "fp16"])
def test_c8_no_grad(mode):
    w, b = params(8, 8, grad=False)
    with torch.no_grad(), profiled(mode) as prof:
        x16 = ops.pack_act16(rnd(1, 8, D, D, D, seed=3), ops._COMPUTE[mode])
        stats = {}
        y16 = ops.conv3d(x16, w, b, c8_out=True, stats=stats)
        y = ops.conv3d(x16, w, b, c8_out=False)
    assert isinstance(y16, ops.Act16) and "partials" in stats and y.dtype == torch.float32
    plan = ops.conv_plan(desc(1, 8, 8, mode), 0)
    check_records(prof, [(FWD, flops(1, 8, 8), plan, nbytes(1, 8, 8, 2, 2)),
                         (FWD, flops(1, 8, 8), plan, nbytes(1, 8, 8, 2, 4))])


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
def test_c8_training(mode, monkeypatch):
    """c8 -> c8 convolution, then the output convolution with its softmax head to 3 fp32 channels; the input carries no
    gradient, so the first convolution has no data gradient: five records"""
    monkeypatch.setattr(ops, "H16_TRAIN_C8ONLY", True)
    monkeypatch.setattr(ops, "_last_scale", ops._last_scale)
    w1, b1 = params(8, 8)
    w2, b2 = params(8, 3, seed=5)
    with profiled(mode) as prof, ops.grad_scale_scope():
        x16 = ops.pack_act16(rnd(1, 8, D, D, D, seed=3), ops._COMPUTE[mode])
        h16 = ops.conv3d(x16, w1, b1, c8_out=True)
        ops.conv3d(h16, w2, b2, softmax=True).sum().backward()
    assert isinstance(h16, ops.Act16)
    d1, d2 = desc(1, 8, 8, mode), desc(1, 8, 3, mode)
    f1, f2 = flops(1, 8, 8), flops(1, 8, 3)
    check_records(prof, [(FWD, f1, ops.conv_plan(d1, 0), nbytes(1, 8, 8, 2, 2)),
                         (FWD, f2, ops.conv_plan(d2, 0), nbytes(1, 8, 3, 2, 4)),
                         (BWW, f2, None, nbytes(1, 8, 3, 2, 2)),
                         (BWD, f2, ops.conv_plan(d2, 1), nbytes(1, 8, 3, 2, 2)),
                         (BWW, f1, None, nbytes(1, 8, 8, 2, 2))])
    assert all(p.grad is not None for p in (w1, b1, w2, b2))


# --------------------------------------------------------------------------------------------------------- gating
def test_gate_keys():
    """CONV_PROFILE_KEYS holding only the forward's (tag, plan): the two gradients are not recorded"""
    N = 2
    x = rnd(N, 8, D, D, D, seed=3).requires_grad_(True)
    w, b = params(8, 8)
    fwd = tensor_flow_expected(N, 8, 8, "fp32")[0]
    with profiled("fp32", keys={(fwd[0], fwd[2])}) as prof:
        ops.conv3d(x, w, b).sum().backward()
    check_records(prof, [fwd])


def test_gate_every():
    """CONV_PROFILE_EVERY = 2 from _prof_seen = 0: the second and the fourth of four forwards"""
    x = rnd(2, 8, D, D, D, seed=3)
    w, b = params(8, 8, grad=False)
    fwd = tensor_flow_expected(2, 8, 8, "fp32")[0]
    with torch.no_grad(), profiled("fp32", every=2) as prof:
        for _ in range(4):
            ops.conv3d(x, w, b)
        assert ops._prof_seen == 4
    check_records(prof, [fwd, fwd])


def test_gate_off():
    """CONV_PROFILE = None: nothing to append to, the list stays None and the launches run"""
    x = rnd(2, 8, D, D, D, seed=3).requires_grad_(True)
    w, b = params(8, 8)
    with profiled("fp32", prof=False) as prof:
        ops.conv3d(x, w, b).sum().backward()
        assert prof is None and ops.CONV_PROFILE is None and ops._prof_seen == 0
    torch.cuda.synchronize()
    assert w.grad is not None


# ------------------------------------------------------------------------------------------------------ the head
@pytest.mark.parametrize("mode", ["fp32", "bf16", "fp16"])
def test_softmax_head_matches_unfused_logits(mode):
    """Whether or not the library fuses the head into the Cout = 3 convolution (the answer is printed), the result is
    softmax of the logits the same call returns without the head, within the suite's 1e-4 of the fp32 mode.  The 16-bit
    modes run the c8 forward, where an unsplit plan has the epilogue: head and logits come from the same fp32
    accumulators there as well, so the bound is the same."""
    w, b = params(8, 3, grad=False, seed=5)
    x = rnd(2, 8, D, D, D, seed=3)
    with torch.no_grad(), profiled(mode, prof=False):
        d = desc(2, 8, 3, mode, *((8 * S, 3 * S) if mode == "fp32" else (0, 0)))
        fuses = _lib.lib().m355_conv3d_fuses_softmax(C.byref(d))
        xin = x if mode == "fp32" else ops.pack_act16(x, ops._COMPUTE[mode])
        logits = ops.conv3d(xin, w, b)
        y = ops.conv3d(xin, w, b, softmax=True)
    err = (y - torch.softmax(logits, dim=1)).abs().max().item()
    print(f"conv_profile softmax head {mode}: fuses_softmax {fuses}  max err {err:.3e}")
    assert fuses in (0, 1)
    assert y.shape == logits.shape and err <= 1e-4
