"""ops._dense_channels / ops._c8t: which gradient layouts reach a kernel as they are, and with which batch stride.

Both helpers are pure Python on tensor metadata (no library, no GPU).  A tensor may be handed to a kernel uncompacted
("aliased") only when its (C, D, H, W) block -- [CB, S, 8] for c8 -- is dense AND its samples do not overlap: for N > 1
the batch stride is at least the sample extent.  The C ABI reads a batch stride of 0 as "dense" (`dense_or`,
csrc/common.hpp), so a batch-expanded gradient (stride 0: what `y.sum(dim=0)` hands its producer) passed through as it
is would make the kernel read N*C*S elements of a C*S buffer.  Everything that does not qualify is compacted and
reported with the dense stride.  The channel slice of a concat buffer MUST stay aliased with the buffer's batch stride:
the models' concat slots rely on it (a copy there is a performance regression on the default path).
"""
import pytest
import torch

from segmentation_pipeline_amd import ops

ALIASED, COMPACTED = "aliased", "compacted"


def _values(*shape):
    return torch.arange(1, 1 + int(torch.tensor(shape).prod()), dtype=torch.float32).reshape(shape)


# (name, builder -> tensor [N, C, D, H, W], verdict, batch stride reported)
NCDHW = [
    ("dense", lambda: _values(2, 3, 2, 4, 4), ALIASED, 96),
    ("n1", lambda: _values(1, 3, 2, 4, 4), ALIASED, 96),
    ("n1_of_a_wider_batch", lambda: _values(4, 3, 2, 4, 4)[1:2], ALIASED, 96),
    ("concat_channel_slice", lambda: _values(2, 8, 2, 4, 4)[:, 3:6], ALIASED, 8 * 32),
    ("concat_channel_slice_first", lambda: _values(2, 8, 2, 4, 4)[:, :3], ALIASED, 8 * 32),
    ("concat_channel_slice_one_channel", lambda: _values(2, 8, 2, 4, 4)[:, 5:6], ALIASED, 8 * 32),
    ("batch_slice_step2", lambda: _values(4, 3, 2, 4, 4)[::2], ALIASED, 2 * 96),
    ("batch_expanded", lambda: _values(1, 3, 2, 4, 4).expand(2, 3, 2, 4, 4), COMPACTED, 96),
    ("batch_expanded_sum_dim0_gradient", lambda: _sum_dim0_gradient(), COMPACTED, 96),
    ("batch_expanded_one_channel", lambda: _values(1, 1, 2, 4, 4).expand(3, 1, 2, 4, 4), COMPACTED, 32),
    ("channel_expanded", lambda: _values(2, 1, 2, 4, 4).expand(2, 3, 2, 4, 4), COMPACTED, 96),
    ("scalar_expanded", lambda: torch.tensor(1.5).expand(2, 3, 2, 4, 4), COMPACTED, 96),
    ("scalar_expanded_sum_gradient", lambda: _sum_gradient(), COMPACTED, 96),
    ("scalar_expanded_all_ones_shape", lambda: torch.tensor(1.5).expand(2, 1, 1, 1, 1), COMPACTED, 1),
    ("permuted_spatial", lambda: _values(2, 3, 4, 4, 2).permute(0, 1, 4, 2, 3), COMPACTED, 96),
    ("permuted_hw", lambda: _values(2, 3, 2, 4, 4).transpose(3, 4), COMPACTED, 96),
    ("w1", lambda: _values(2, 3, 2, 4, 1), ALIASED, 24),
    ("w1_of_a_wider_row", lambda: _values(2, 3, 2, 4, 5)[..., 2:3], COMPACTED, 24),
    ("h1", lambda: _values(2, 3, 2, 1, 4), ALIASED, 24),
    ("d1", lambda: _values(2, 3, 1, 4, 4), ALIASED, 48),
    ("d1_slice_of_a_deeper_volume", lambda: _values(2, 3, 2, 4, 4)[:, :, 1:2], COMPACTED, 48),
    ("d1_h1_w1", lambda: _values(2, 3, 1, 1, 1), ALIASED, 3),
    ("d1_batch_expanded", lambda: _values(1, 3, 1, 4, 4).expand(2, 3, 1, 4, 4), COMPACTED, 48),
    ("overlapping_as_strided_batch", lambda: torch.as_strided(_values(200), (2, 3, 2, 4, 4), (40, 32, 16, 4, 1)),
     COMPACTED, 96),
    ("as_strided_batch_touching", lambda: torch.as_strided(_values(200), (2, 3, 2, 4, 4), (96, 32, 16, 4, 1), 5),
     ALIASED, 96),
]


def _sum_dim0_gradient():
    """the gradient autograd hands the producer of a tensor consumed by `.sum(dim=0)`, caught by a hook"""
    caught = []
    y = _values(2, 3, 2, 4, 4).requires_grad_(True)
    z = y * 1.0
    z.register_hook(lambda g: caught.append(g))
    (z.sum(dim=0) * _values(3, 2, 4, 4)).sum().backward()
    return caught[0]


def _sum_gradient():
    caught = []
    y = _values(2, 3, 2, 4, 4).requires_grad_(True)
    z = y * 1.0
    z.register_hook(lambda g: caught.append(g))
    z.sum().backward()
    return caught[0]


def _c8_values(*shape):
    return _values(*shape).to(torch.bfloat16)


# the same table for c8 tensors [N, CB, S, 8]
C8 = [
    ("dense", lambda: _c8_values(2, 2, 6, 8), ALIASED, 96),
    ("n1", lambda: _c8_values(1, 2, 6, 8), ALIASED, 96),
    ("concat_block_slice", lambda: _c8_values(2, 5, 6, 8)[:, 1:3], ALIASED, 5 * 48),
    ("concat_block_slice_one_block", lambda: _c8_values(2, 5, 6, 8)[:, 4:5], ALIASED, 5 * 48),
    ("batch_slice_step2", lambda: _c8_values(4, 2, 6, 8)[::2], ALIASED, 2 * 96),
    ("batch_expanded", lambda: _c8_values(1, 2, 6, 8).expand(2, 2, 6, 8), COMPACTED, 96),
    ("batch_expanded_one_block", lambda: _c8_values(1, 1, 6, 8).expand(2, 1, 6, 8), COMPACTED, 48),
    ("block_expanded", lambda: _c8_values(2, 1, 6, 8).expand(2, 2, 6, 8), COMPACTED, 96),
    ("scalar_expanded", lambda: torch.tensor(1.5, dtype=torch.bfloat16).expand(2, 2, 6, 8), COMPACTED, 96),
    ("permuted_s_and_lane", lambda: _c8_values(2, 2, 8, 6).transpose(2, 3), COMPACTED, 96),
    ("s1", lambda: _c8_values(2, 2, 1, 8), ALIASED, 16),
    ("overlapping_as_strided_batch", lambda: torch.as_strided(_c8_values(400), (2, 2, 6, 8), (48, 48, 8, 1)),
     COMPACTED, 96),
    ("misaligned_batch_stride", lambda: torch.as_strided(_c8_values(400), (2, 2, 6, 8), (100, 48, 8, 1)),
     COMPACTED, 96),
    ("fp16_batch_expanded", lambda: _values(1, 2, 6, 8).to(torch.float16).expand(3, 2, 6, 8), COMPACTED, 96),
]


def _check(helper, build, verdict, batch_stride):
    t = build()
    before = t.clone()
    r, bs = helper(t)
    assert torch.equal(r, t) and torch.equal(t, before)
    assert tuple(r.shape) == tuple(t.shape) and r.dtype == t.dtype
    assert bs == batch_stride
    n = t.shape[0]
    extent = t[0].numel()
    if verdict == ALIASED:
        assert r.data_ptr() == t.data_ptr() and r.stride() == t.stride()
    else:
        assert r.is_contiguous() and r.data_ptr() != t.data_ptr()
    # what a kernel may assume of (tensor, batch stride), whichever the verdict: sample n starts `bs` elements after
    # sample n - 1, samples do not overlap, and every sample is dense
    assert n == 1 or bs >= extent
    for i in range(n):
        flat = torch.as_strided(r, (extent,), (1,), r.storage_offset() + i * bs)
        assert torch.equal(flat, before[i].reshape(-1)), f"sample {i} read with batch stride {bs}"


@pytest.mark.parametrize("name,build,verdict,batch_stride", NCDHW, ids=[r[0] for r in NCDHW])
def test_dense_channels_layouts(name, build, verdict, batch_stride):
    _check(ops._dense_channels, build, verdict, batch_stride)


@pytest.mark.parametrize("name,build,verdict,batch_stride", C8, ids=[r[0] for r in C8])
def test_c8t_layouts(name, build, verdict, batch_stride):
    _check(ops._c8t, build, verdict, batch_stride)


def test_sum_dim0_gradient_really_has_batch_stride_zero():
    """the premise of the batch-expanded rows: autograd does hand over stride 0 for `y.sum(dim=0)`"""
    g = _sum_dim0_gradient()
    assert g.stride() == (0, 32, 16, 4, 1)
    assert all(s == 0 for s in _sum_gradient().stride())
