"""DeepSupervisionUNet: ModularUNet with auxiliary segmentation heads on its coarser decoder levels.

Deep supervision (nnU-Net's training scheme): besides the full-resolution output, the decoder levels 1..k -- the outputs
of `up_blocks[1..k]`, `filters[i]` channels at the input size / 2^i -- each get an output convolution of their own and the
model's hypothesis, and are trained against a down-scaled target (`criterions.DeepSupervisionLoss`, `ops.target_pyramid`).
Small targets then reach the deep levels with a gradient of their own.

Not part of the reference: `ModularUNet.__init__` keeps the reference's argument list, the feature is this subclass with
one keyword-only argument.  The heads are created after every module of ModularUNet, so under one seed the shared
parameters draw ModularUNet's values, ModularUNet's state_dict keys are a strict subset, and a reference checkpoint loads
with strict=False, missing exactly `aux_convs.*`.

In eval mode no head runs: `forward` returns one tensor, the launches are ModularUNet's, the result has its bits.  In
training mode `forward` returns the tuple (y_pred, aux_1, ..., aux_k), finest first.
"""
from torch import nn

from .. import ops
from .components import _check_conv_module
from .modular_unet import ModularUNet

MAX_AUX_LEVELS = ops.PYRAMID_MAX_LEVELS   # what one ops.target_pyramid launch writes


class DeepSupervisionUNet(ModularUNet):
    def __init__(self, *args, aux_levels=None, **kwargs):
        super().__init__(*args, **kwargs)
        depth, filters = self.depth, self._filters
        if aux_levels is None:
            aux_levels = depth - 2       # every decoder level below the output's
        most = min(depth - 2, MAX_AUX_LEVELS)
        if isinstance(aux_levels, bool) or not isinstance(aux_levels, int) or not 1 <= aux_levels <= most:
            raise ValueError(f"aux_levels = {aux_levels!r}: a model of depth {depth} has decoder levels 1..{depth - 2} "
                             f"below its output, and at most {MAX_AUX_LEVELS} are supervised "
                             f"(expected 1 <= aux_levels <= {most})" if most >= 1 else
                             f"aux_levels = {aux_levels!r}: a model of depth {depth} has no decoder level below its output")
        self.aux_levels = aux_levels

        # the arguments ModularUNet built out_conv from (positional or keyword), its default dict when none was given
        names = ("in_channels", "out_channels", "filters", "depth", "block_class", "block_params", "upsample_class",
                 "upsample_params", "downsample_class", "downsample_params", "out_conv_class", "out_conv_params")
        given = dict(zip(names, args))
        given.update(kwargs)
        out_conv_class = given.get("out_conv_class", nn.Conv3d)
        out_conv_params = given.get("out_conv_params")
        if out_conv_params is None:
            out_conv_params = {'in_channels': filters[0], 'out_channels': given["out_channels"], 'kernel_size': 3,
                               'padding': 1}
        # created AFTER every module of ModularUNet: the shared parameters keep their seeded values
        self.aux_convs = nn.ModuleList()
        for i in range(1, aux_levels + 1):
            conv = out_conv_class(**{**out_conv_params, 'in_channels': filters[i]})
            _check_conv_module(conv)
            self.aux_convs.append(conv)

    def forward(self, x):
        if not self.training:
            return super().forward(x)
        with ops.grad_scale_scope():
            aux = [None] * self.aux_levels
            y_pred = self._forward(x, aux)
        return (y_pred, *aux)

    def _decoder_level(self, i, x, levels):
        # Runs inside the decoder loop, so every auxiliary head is recorded BEFORE the output convolution.  Autograd runs
        # the node created last first: the full-resolution head's backward is the first head backward of a pass and
        # resolves its fp16 loss scale (ops.GradScale.resolve), as it does in ModularUNet; the auxiliary heads read it.
        if levels is not None and i <= self.aux_levels:
            levels[i - 1] = self._head(self.aux_convs[i - 1], x)
