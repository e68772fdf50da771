"""The fp64 torch restatements of tests/autograd_cases.py against the C oracle (CPU only).

tests/test_autograd_contract_gpu.py holds the ops to the tolerances the kernel tests apply against the C oracle, but
measures against fp64 torch autograd.  The oracle accumulates in double, so the two references must agree far inside those
tolerances: for every op with an oracle entry, every output and every gradient of the restatement is within ONE TENTH of
the tolerance of the oracle's on the same seeded inputs.  A restatement that misses this is wrong.
"""
import pytest
import torch

import autograd_cases as A

WITH_ORACLE = [c for c in A.CASES if c.oracle is not None]


@pytest.mark.parametrize("case", WITH_ORACLE, ids=lambda c: c.name)
def test_fp64_restatement_agrees_with_the_c_oracle(oracle, case):
    ref = A.reference(case)
    t = {**case.inputs, **case.consts}
    got = case.oracle(oracle, t, ref["dys"])
    want = {f"out{i}": o for i, o in enumerate(ref["outs"])}
    want.update(ref["grads"])
    assert got, "an oracle entry that returns nothing"
    rows = []
    for key, value in got.items():
        assert want[key] is not None, key
        ratio = A.excess(case, key, value, want[key], ref)
        rows.append(f"{key} {ratio:.2g}")
        assert ratio <= 0.1, f"{case.name} {key}: oracle vs fp64 restatement at {ratio:.3g} of the tolerance"
    print(f"{case.name}: oracle vs fp64, fraction of the tolerance: " + ", ".join(rows))


def test_every_op_family_of_the_issue_is_in_the_table():
    names = " ".join(c.name for c in A.CASES)
    for op in ("conv3d_", "conv_transpose3d", "norm_act_gn", "norm_act_bn_train", "norm_act_bn_eval", "norm_act_pool",
               "avgpool3d_2x_r", "avgpool3d_2x_with_skip", "maxpool3d_2x_r", "maxpool3d_2x_with_skip", "upsample_trilinear2x_r",
               "upsample_nearest2x", "upsample_trilinear2x_hp", "softmax_channels_inner1", "softmax_channels_inner_c", "sigmoid",
               "hybrid_logistic_dice_loss", "channel_scale", "add_", "copy_into", "space_to_depth2", "depth_to_space2",
               "blur_weight", "weight_standardize"):
        assert op in names, op
    for c in A.CASES:
        assert all(v.shape[0] == A.N for k, v in c.inputs.items() if v.dim() == 5 and k not in ("w",)), c.name
        assert set(c.tol) >= set(c.inputs) | {"out0"}, c.name


def test_restatement_gradients_are_complete():
    """every differentiable input of every case gets a gradient from the fp64 restatement"""
    for c in A.CASES:
        ref = A.reference(c)
        for k, g in ref["grads"].items():
            assert g is not None and g.shape == c.inputs[k].shape and bool(torch.isfinite(g).all()), (c.name, k)
