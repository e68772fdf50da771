"""TEST HELPER -- the table of differentiable public ops of segmentation_pipeline_amd.ops that
tests/test_autograd_contract_gpu.py drives on the device and tests/test_autograd_refs_cpu.py checks on the CPU.

A `Case` is one call of one op through its public function:
  inputs   name -> seeded fp32 CPU tensor, every one of them differentiable
  consts   name -> CPU tensor that takes no gradient (targets, masks, running statistics, scales)
  run(t)   the call through `ops` on device tensors (t holds inputs and consts) -> output tensor or tuple
  ref(t)   the same operation restated with torch.nn.functional on float64 CPU tensors
  tol      "out0", "out1", ... and every input name -> (rtol, atol) of tests/test_kernels_gpu.py's close():
           max |got - ref| <= atol + rtol * max |ref|, or a callable (t64, dys64) -> per-element absolute bound
  plans    precision mode -> the (forward, data-gradient, weight-gradient) kernel families m355_conv3d_plan must report
  oracle   (RawOps("oracle"), fp32 inputs and consts, fp32 dys) -> the same names as `tol`, through the C oracle

Every tolerance is the one tests/test_kernels_gpu.py (K below), tests/test_sigmoid_head_gpu.py (SG) or
tests/test_upsample_modes_gpu.py (UP) applies to the same kernel against the C oracle; the line is cited next to it.
"""
import torch
import torch.nn.functional as F

import upsample_ref as U
from oracle import torch_ref as R
from segmentation_pipeline_amd import ops

N = 2                      # throughout: the batch stride only matters for N > 1
EXACT = (0.0, 0.0)
ONE_ROUNDING = (2.0 ** -24, 0.0)   # one fp32 operation on exact operands, against its exact value
ULP = 2.0 ** -24


def rnd(*shape, seed=0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


class Case:
    def __init__(self, name, inputs, run, ref, tol, consts=None, plans=None, desc=None, oracle=None):
        self.name, self.inputs, self.consts = name, inputs, consts or {}
        self.run, self.ref, self.tol, self.plans, self.desc, self.oracle = run, ref, tol, plans, desc, oracle

    def __repr__(self):
        return self.name


def _tuple(o):
    return tuple(o) if isinstance(o, (tuple, list)) else (o,)


# ----------------------------------------------------------------------------------------------------------- conv3d
# K:52-59 (test_conv3d_3x3x3_fwd_bwd) and K:98-103 (test_conv3d_f32x3_fwd_bwd): forward and data gradient close(2e-5, 2e-5),
# weight and bias gradient close(3e-5, 3e-5 * sqrt(N * D * H * W)).  The fused `add` takes the incoming gradient as it is.
def _conv_tol(D, H, W, names, head=None):
    vox = 3e-5 * (N * D * H * W) ** 0.5
    # K:392 (test_out_conv_softmax_fused_epilogue) / SG:126: conv + head close(2e-5, 1e-6)
    tol = {"out0": (2e-5, 1e-6) if head else (2e-5, 2e-5)}
    for n in names:
        tol[n] = {"w": (3e-5, vox), "bias": (3e-5, vox), "add": EXACT}.get(n, (2e-5, 2e-5))
    return tol


def _conv_oracle(parts, head):
    def oracle(O, t, dys):
        x = torch.cat([t[p] for p in parts], dim=1)
        w, b, add = t["w"], t.get("bias"), t.get("add")
        y = O.conv3d_fwd(x, w, b, add)
        dy = dys[0]
        if head == "softmax":
            y = O.softmax_fwd(y)
            dy = O.softmax_bwd(y, dy)
        elif head == "sigmoid":    # (the oracle library has no sigmoid entry: SG:126 applies torch's to its logits, in double)
            y = torch.sigmoid(y.double())
            dy = (dy.double() * y * (1.0 - y)).float()
        out = {"out0": y}
        dx = O.conv3d_bwd_data(dy, w, x.shape)
        c0 = 0
        for p in parts:
            out[p] = dx[:, c0:c0 + t[p].shape[1]]
            c0 += t[p].shape[1]
        out["w"], db = O.conv3d_bwd_weight(x, dy, 3, with_bias=b is not None)
        if b is not None:
            out["bias"] = db
        if add is not None:
            out["add"] = dy
        return out
    return oracle


def conv_case(name, cin_parts, cout, spatial, plans, bias=True, add=False, head=None):
    D, H, W = spatial
    cin = sum(cin_parts)
    parts = ["x"] if len(cin_parts) == 1 else [f"part{i}" for i in range(len(cin_parts))]
    inputs = {p: rnd(N, c, D, H, W, seed=11 + i) for i, (p, c) in enumerate(zip(parts, cin_parts))}
    inputs["w"] = rnd(cout, cin, 3, 3, 3, seed=2) * (1.0 / (27 * cin) ** 0.5)
    if bias:
        inputs["bias"] = rnd(cout, seed=3)
    if add:
        inputs["add"] = rnd(N, cout, D, H, W, seed=4)

    def run(t):
        kw = dict(add=t.get("add"), softmax=head == "softmax", sigmoid=head == "sigmoid")
        if len(parts) == 1:
            return ops.conv3d(t["x"], t["w"], t.get("bias"), **kw)
        # the parts live in adjacent channel slices of one buffer, as the models' producers leave them
        buf = torch.empty((N, cin, D, H, W), dtype=torch.float32, device=t["w"].device)
        c0, slots = 0, []
        for p, c in zip(parts, cin_parts):
            slots.append(ops.copy_into(t[p], ops.OutSlot(buf, c0, c0 + c)))
            c0 += c
        return ops.conv3d(ops.Concat(buf, slots), t["w"], t.get("bias"), **kw)

    def ref(t):
        y = F.conv3d(torch.cat([t[p] for p in parts], dim=1), t["w"], t.get("bias"), padding=1)
        if add:
            y = y + t["add"]
        return torch.softmax(y, dim=1) if head == "softmax" else (torch.sigmoid(y) if head == "sigmoid" else y)

    return Case(name, inputs, run, ref, _conv_tol(D, H, W, list(inputs), head), plans=plans,
                desc=(cin, cout, D, H, W), oracle=_conv_oracle(parts, head))


# (forward, data gradient, weight gradient) families of m355_conv3d_plan: 1 fp32 MFMA, 2 small-Cout forward, 7 split
# (three bf16 planes) forward / data gradient, 8 split weight gradient, 9 fp32 MFMA / vector weight gradient, 10 the
# edge layers' weight gradient (<= 4 channels on one side)
EDGE = {"fp32": (1, 1, 10), "fp32_mfma": (1, 1, 10)}
OUT = {"fp32": (2, 1, 10), "fp32_mfma": (2, 1, 10)}
WIDE = {"fp32": (7, 7, 8), "fp32_mfma": (1, 1, 9)}

CONV = [
    conv_case("conv3d_first_layer", [3], 16, (5, 6, 9), EDGE),                         # small Cin, ragged, W % 4 != 0
    conv_case("conv3d_first_layer_nobias", [3], 16, (5, 6, 9), EDGE, bias=False),
    conv_case("conv3d_out", [9], 3, (8, 5, 33), OUT),                                  # small-Cout forward kernel, odd Cin
    conv_case("conv3d_out_softmax_fused", [9], 3, (8, 5, 33), OUT, head="softmax"),    # head in the conv epilogue
    conv_case("conv3d_out_sigmoid_fused", [9], 3, (8, 5, 33), OUT, head="sigmoid"),
    conv_case("conv3d_out_softmax_unfused", [16], 3, (6, 6, 12), EDGE, head="softmax"),   # W < 32: MFMA + a softmax pass
    conv_case("conv3d_out_sigmoid_unfused_nobias", [16], 3, (6, 6, 12), EDGE, head="sigmoid", bias=False),
    conv_case("conv3d_wide", [20], 24, (5, 6, 9), WIDE),                               # channel remainders on both sides
    conv_case("conv3d_wide_nobias", [20], 24, (5, 6, 9), WIDE, bias=False),
    conv_case("conv3d_wide_add", [20], 24, (5, 6, 9), WIDE, add=True),                 # fused residual
    conv_case("conv3d_wide_add_nobias", [20], 24, (5, 6, 9), WIDE, add=True, bias=False),
    conv_case("conv3d_wide_w32", [12], 40, (8, 8, 32), WIDE),                          # 32-wide x tiles, vectorisable
    conv_case("conv3d_concat_5_16", [5, 16], 16, (6, 8, 8), WIDE),                     # first part no multiple of 8
    conv_case("conv3d_concat_8_8_add", [8, 8], 8, (4, 6, 8), WIDE, add=True),          # equal parts (offsets can be confused)
]


# ------------------------------------------------------------------------------------------------- conv_transpose3d
def convt_case(name, cin, cout, spatial, bias):
    D, H, W = spatial
    inputs = {"x": rnd(N, cin, D, H, W, seed=1), "w": rnd(cin, cout, 2, 2, 2, seed=2) * (1.0 / (8 * cin) ** 0.5)}
    if bias:
        inputs["bias"] = rnd(cout, seed=3)

    def oracle(O, t, dys):
        out = {"out0": O.convt_fwd(t["x"], t["w"], t.get("bias")), "x": O.convt_bwd_data(dys[0], t["w"], t["x"].shape)}
        out["w"], db = O.convt_bwd_weight(t["x"], dys[0], 2, with_bias=bias)
        if bias:
            out["bias"] = db
        return out
    # K:468-474 (test_conv_transpose3d_fwd_bwd): forward and data gradient close(2e-5, 2e-5), weight / bias close(3e-5, 1e-4)
    tol = {"out0": (2e-5, 2e-5), "x": (2e-5, 2e-5), "w": (3e-5, 1e-4), "bias": (3e-5, 1e-4)}
    return Case(name, inputs, lambda t: ops.conv_transpose3d(t["x"], t["w"], t.get("bias")),
                lambda t: F.conv_transpose3d(t["x"], t["w"], t.get("bias"), stride=2), tol, oracle=oracle)


CONVT = [convt_case("conv_transpose3d", 12, 20, (3, 5, 7), True),              # ragged, odd sizes
         convt_case("conv_transpose3d_nobias", 16, 8, (4, 4, 8), False)]       # vectorisable


# --------------------------------------------------------------------------------------------------------- norm_act
RELU, LEAKY = 1, 2


def _act(y, act):
    return F.relu(y) if act == RELU else (F.leaky_relu(y, 0.01) if act == LEAKY else y)


def _norm_ref(t, groups, training, act):
    if groups:
        y = F.group_norm(t["x"], groups, t["gamma"], t["beta"], 1e-5)
    else:
        y = F.batch_norm(t["x"], None if training else t["running_mean"].clone(), None if training else t["running_var"].clone(),
                         t["gamma"], t["beta"], training, 0.1, 1e-5)
    return _act(y, act)


def _norm_stats_oracle(O, t, groups, training):
    if groups or training:
        return O.norm_stats(t["x"], groups)[:2]
    return t["running_mean"], (t["running_var"].double() + 1e-5).rsqrt().float()


def norm_case(name, C, spatial, groups, act, training=True, add=False, pool=False):
    D, H, W = spatial
    inputs = {"x": rnd(N, C, D, H, W, seed=1) * 1.7 + 0.3, "gamma": rnd(C, seed=2), "beta": rnd(C, seed=3)}
    if add:
        inputs["add"] = rnd(N, C, D, H, W, seed=4)
    consts = {}
    if not groups:
        consts = {"running_mean": rnd(C, seed=5) * 0.1, "running_var": torch.rand(C, generator=torch.Generator().manual_seed(6)) + 0.5}

    def cfg(t):
        return ops.NormCfg(groups=groups, eps=1e-5, act=act, slope=0.01, training=training,
                           running_mean=t.get("running_mean"), running_var=t.get("running_var"))

    def run(t):
        if pool:
            return ops.norm_act_pool(t["x"], t["gamma"], t["beta"], cfg(t))
        return ops.norm_act(t["x"], t["gamma"], t["beta"], cfg(t), add=t.get("add"))

    def ref(t):
        y = _norm_ref(t, groups, training, act)
        if pool:
            return y, F.avg_pool3d(y, 2, 2)
        return y + t["add"] if add else y

    def oracle(O, t, dys):
        mean, rstd = _norm_stats_oracle(O, t, groups, training)
        y = O.norm_act_fwd(t["x"], mean, rstd, t["gamma"], t["beta"], groups, act, t.get("add"))
        dy = dys[0]
        out = {"out0": y}
        if pool:
            out["out1"] = O.avgpool_fwd(y)
            dy = O.avgpool_bwd_add(dys[1], dys[0], y.shape)
        out["x"], out["gamma"], out["beta"] = O.norm_act_bwd(t["x"], dy, mean, rstd, t["gamma"], t["beta"], groups, act,
                                                             1 if (groups or training) else 0)
        if add:
            out["add"] = dys[0]
        return out
    # K:520-528 (test_norm_act_fwd_bwd): forward close(2e-5, 2e-5), dx close(2e-5, 2e-5), dgamma / dbeta close(2e-5, 1e-4);
    # K:871 (test_norm_act_with_pooled_second_output): pooled close(1e-5, 1e-6).  `add` takes the incoming gradient as it is.
    tol = {"out0": (2e-5, 2e-5), "out1": (1e-5, 1e-6), "x": (2e-5, 2e-5), "gamma": (2e-5, 1e-4), "beta": (2e-5, 1e-4), "add": EXACT}
    return Case(name, inputs, run, ref, tol, consts=consts, oracle=oracle)


NORM = [
    norm_case("norm_act_gn_ragged", 16, (5, 6, 7), 4, RELU),                    # S % 4 != 0: the scalar path
    norm_case("norm_act_gn_add", 8, (4, 6, 8), 2, LEAKY, add=True),
    norm_case("norm_act_gn_ragged_add", 6, (3, 3, 5), 3, RELU, add=True),
    norm_case("norm_act_bn_train", 8, (4, 6, 8), 0, RELU),
    norm_case("norm_act_bn_train_ragged_add", 6, (3, 3, 5), 0, LEAKY, add=True),
    norm_case("norm_act_bn_eval", 8, (4, 6, 8), 0, RELU, training=False),
    norm_case("norm_act_bn_eval_ragged_add", 6, (3, 3, 5), 0, LEAKY, training=False, add=True),
    norm_case("norm_act_pool_gn", 8, (4, 6, 8), 2, RELU, pool=True),
    norm_case("norm_act_pool_bn_w_not_4", 6, (2, 6, 10), 0, LEAKY, pool=True),      # even sizes, W % 4 != 0
]


# ---------------------------------------------------------------------------------------------------- pools, upsampling
def _simple(name, shape, run, ref, tol, oracle=None, seed=1, consts=None):
    return Case(name, {"x": rnd(*shape, seed=seed)}, run, ref, tol, consts=consts, oracle=oracle)


def _pool_cases():
    cases = []
    for tag, shape in (("ragged", (N, 5, 2, 6, 10)), ("vec", (N, 4, 4, 8, 16))):     # W/2 odd: one output per thread
        # K:535-537 (test_pool_upsample_softmax): forward close(1e-6, 1e-6), backward close(0, 0);
        # K:557 (test_avgpool_bwd_fused_with_skip_gradient): skip + un-pooled gradient close(0, 1e-7)
        cases.append(_simple(f"avgpool3d_2x_{tag}", shape, lambda t: ops.avgpool3d_2x(t["x"]), lambda t: F.avg_pool3d(t["x"], 2, 2),
                             {"out0": (1e-6, 1e-6), "x": EXACT},
                             oracle=lambda O, t, dys: {"out0": O.avgpool_fwd(t["x"]), "x": O.avgpool_bwd(dys[0], t["x"].shape)}))
        cases.append(_simple(f"avgpool3d_2x_with_skip_{tag}", shape, lambda t: ops.avgpool3d_2x_with_skip(t["x"]),
                             lambda t: (t["x"] * 1.0, F.avg_pool3d(t["x"], 2, 2)), {"out0": EXACT, "out1": (1e-6, 1e-6), "x": (0.0, 1e-7)},
                             oracle=lambda O, t, dys: {"out0": t["x"], "out1": O.avgpool_fwd(t["x"]),
                                                       "x": O.avgpool_bwd_add(dys[1], dys[0], t["x"].shape)}))
        # tests/test_maxpool_gpu.py: value, route and gradient are stock torch's bit for bit; with the skip gradient the
        # one fp32 addition per element is the bound of the average pool's fused sum (K:557)
        cases.append(_simple(f"maxpool3d_2x_{tag}", shape, lambda t: ops.maxpool3d_2x(t["x"]), lambda t: F.max_pool3d(t["x"], 2, 2),
                             {"out0": EXACT, "x": EXACT}))
        cases.append(_simple(f"maxpool3d_2x_with_skip_{tag}", shape, lambda t: ops.maxpool3d_2x_with_skip(t["x"]),
                             lambda t: (t["x"] * 1.0, F.max_pool3d(t["x"], 2, 2)), {"out0": EXACT, "out1": EXACT, "x": (0.0, 1e-7)}))
    return cases


def _upsample_cases():
    cases = []
    for tag, shape in (("ragged", (N, 3, 3, 4, 5)), ("vec", (N, 2, 4, 4, 8))):
        # K:543-545 (test_pool_upsample_softmax): forward close(2e-6, 2e-6), backward close(1e-5, 1e-5)
        cases.append(_simple(f"upsample_trilinear2x_{tag}", shape, lambda t: ops.upsample_trilinear2x(t["x"]),
                             lambda t: U.upsample(t["x"], "trilinear"), {"out0": (2e-6, 2e-6), "x": (1e-5, 1e-5)},
                             oracle=lambda O, t, dys: {"out0": O.upsample_fwd(t["x"]), "x": O.upsample_bwd(dys[0], t["x"].shape)}))
        # UP:132-143 (test_fp32_nearest_kernels): the forward copies bits; |dx - dx64| <= 7 * 2^-24 * sum |dy| over the block
        cases.append(_simple(f"upsample_nearest2x_{tag}", shape, lambda t: ops.upsample_nearest2x(t["x"]),
                             lambda t: U.upsample(t["x"], "nearest"),
                             {"out0": EXACT, "x": lambda t, dys: 7 * ULP * U.upsample_grad(dys[0].abs(), "nearest", t["x"].shape)}))
        # UP:149-167 (test_fp32_half_pixel_kernels): |y - y64| <= 10 * 2^-24 * max |x| over the 3x3x3 neighbourhood,
        # |dx - dx64| <= 66 * 2^-24 * sum |w * dy| over the contributing outputs
        cases.append(_simple(f"upsample_trilinear2x_hp_{tag}", shape, lambda t: ops.upsample_trilinear2x_hp(t["x"]),
                             lambda t: U.upsample(t["x"], "trilinear_hp"),
                             {"out0": lambda t, dys: 10 * ULP * U.neighbourhood_max(t["x"]),
                              "x": lambda t, dys: 66 * ULP * U.upsample_grad(dys[0].abs(), "trilinear_hp", t["x"].shape)}))
    return cases


# ------------------------------------------------------------------------------------------- softmax, sigmoid, loss
def _stochastic_ref(x, C, bias):
    n, sp = x.shape[0], x.shape[2:]
    x = x.reshape(n, C, C, *sp) + torch.eye(C, dtype=x.dtype).reshape(1, C, C, *(1 for _ in sp)) * bias
    return torch.softmax(x, dim=1).reshape(n, C * C, *sp)


def _softmax_oracle(inner, bias):
    def oracle(O, t, dys):
        y = O.softmax_fwd(t["x"], inner, bias)
        return {"out0": y, "x": O.softmax_bwd(y, dys[0], inner)}
    return oracle


def _head_cases():
    # K:550-552 (test_pool_upsample_softmax): softmax forward close(2e-6, 1e-7), backward close(1e-5, 1e-6)
    sm = {"out0": (2e-6, 1e-7), "x": (1e-5, 1e-6)}
    cases = [
        Case("softmax_channels_inner1", {"x": rnd(N, 7, 3, 5, 6, seed=5) * 3}, lambda t: ops.softmax_channels(t["x"]),
             lambda t: torch.softmax(t["x"], dim=1), sm, oracle=_softmax_oracle(1, 0.0)),
        Case("softmax_channels_inner_c", {"x": rnd(N, 9, 4, 4, 8, seed=5) * 3}, lambda t: ops.softmax_channels(t["x"], inner=3, diag_bias=5.0),
             lambda t: _stochastic_ref(t["x"], 3, 5.0), sm, oracle=_softmax_oracle(3, 5.0)),
        # SG:74-76: sigmoid forward and backward close(2e-5, 1e-6)
        Case("sigmoid", {"x": rnd(N, 3, 3, 5, 7, seed=6) * 3}, lambda t: ops.sigmoid(t["x"]), lambda t: torch.sigmoid(t["x"]),
             {"out0": (2e-5, 1e-6), "x": (2e-5, 1e-6)}),
    ]
    for tag, shape, dw, cw, sq in (("ragged", (N, 3, 5, 6, 7), 0.5, None, True), ("weights", (N, 3, 4, 4, 8), 0.3, [1.0, 2.0, 3.0], False)):
        p = torch.softmax(rnd(*shape, seed=1) * 2, dim=1)
        lab = torch.randint(0, 3, (N,) + shape[2:], generator=torch.Generator().manual_seed(2))
        consts = {"target": F.one_hot(lab, 3).permute(0, 4, 1, 2, 3).float().contiguous()}
        if cw is not None:
            consts["cw"] = torch.tensor(cw)

        def run(t, dw=dw, sq=sq):
            return ops.hybrid_logistic_dice_loss(t["p"], t["target"], dw, t.get("cw"), sq)[0]

        def ref(t, dw=dw, cw=cw, sq=sq):
            return R.hybrid_logistic_dice_loss(t["p"], t["target"], dw, cw, sq)["loss"]

        def oracle(O, t, dys, dw=dw, sq=sq):
            out3, sums = O.loss_fwd(t["p"], t["target"], dw, t.get("cw"), sq)
            return {"out0": out3[0], "p": O.loss_bwd(t["p"], t["target"], sums, float(dys[0]), dw, t.get("cw"), sq)}
        # K:646-648 (test_hybrid_loss_fwd_bwd): loss close(2e-6, 1e-7), dp close(1e-5, 1e-9)
        cases.append(Case(f"hybrid_logistic_dice_loss_{tag}", {"p": p}, run, ref, {"out0": (2e-6, 1e-7), "p": (1e-5, 1e-9)},
                          consts=consts, oracle=oracle))
    return cases


# -------------------------------------------------------------------------------------------------------- elementwise
def _s2d_ref(x):
    n, c, d, h, w = x.shape
    return x.reshape(n, c, d // 2, 2, h // 2, 2, w // 2, 2).permute(0, 1, 3, 5, 7, 2, 4, 6).reshape(n, c * 8, d // 2, h // 2, w // 2)


def _d2s_ref(x):
    n, c8, d, h, w = x.shape
    return x.reshape(n, c8 // 8, 2, 2, 2, d, h, w).permute(0, 1, 5, 2, 6, 3, 7, 4).reshape(n, c8 // 8, 2 * d, 2 * h, 2 * w)


def _copy_into(t):
    x = t["x"]
    buf = torch.zeros((x.shape[0], x.shape[1] + 5) + tuple(x.shape[2:]), dtype=torch.float32, device=x.device)
    return ops.copy_into(x, ops.OutSlot(buf, 3, 3 + x.shape[1]))


def _elementwise_cases():
    cases = []
    for tag, shape in (("ragged", (N, 5, 3, 5, 7)), ("vec", (N, 4, 4, 4, 8))):
        scale = torch.rand(shape[0] * shape[1], generator=torch.Generator().manual_seed(8)).gt(0.3).float() / 0.7
        # one fp32 multiplication (addition) of exact operands per element
        cases.append(_simple(f"channel_scale_{tag}", shape, lambda t: ops.channel_scale(t["x"], t["scale"]),
                             lambda t: t["x"] * t["scale"].reshape(t["x"].shape[0], t["x"].shape[1], 1, 1, 1),
                             {"out0": ONE_ROUNDING, "x": ONE_ROUNDING}, consts={"scale": scale}))
        cases.append(Case(f"add_{tag}", {"a": rnd(*shape, seed=1), "b": rnd(*shape, seed=2)}, lambda t: ops.add(t["a"], t["b"]),
                          lambda t: t["a"] + t["b"], {"out0": ONE_ROUNDING, "a": EXACT, "b": EXACT}))
        # copies and permutations: bits (K:566, test_space_to_depth_roundtrip)
        cases.append(_simple(f"copy_into_{tag}", shape, _copy_into, lambda t: t["x"] * 1.0, {"out0": EXACT, "x": EXACT},
                             oracle=lambda O, t, dys: {"out0": O.copy_channels(t["x"]), "x": dys[0]}))
    for tag, shape in (("w_not_4", (N, 3, 2, 6, 10)), ("vec", (N, 2, 4, 4, 16))):
        cases.append(_simple(f"space_to_depth2_{tag}", shape, lambda t: ops.space_to_depth2(t["x"]), lambda t: _s2d_ref(t["x"]),
                             {"out0": EXACT, "x": EXACT},
                             oracle=lambda O, t, dys: {"out0": O.space_to_depth(t["x"]), "x": O.depth_to_space(dys[0])}))
        s2 = (shape[0], shape[1] * 8, shape[2] // 2, shape[3] // 2, shape[4] // 2)
        cases.append(_simple(f"depth_to_space2_{tag}", s2, lambda t: ops.depth_to_space2(t["x"]), lambda t: _d2s_ref(t["x"]),
                             {"out0": EXACT, "x": EXACT},
                             oracle=lambda O, t, dys: {"out0": O.depth_to_space(t["x"]), "x": O.space_to_depth(dys[0])}))
    return cases


# ---------------------------------------------------------------------------------------------- weight transforms
def _blur_ref(w, scale, standardize, transposed):
    """the reference's Blur filter (components.py:112-119 / 145-152: optional standardisation, the depthwise 2x2x2 box
    blur with padding 1 -> 4x4x4 / stride 2 / padding 1) rearranged into the 3x3x3 filter of the space-to-depth form:
    strided conv      out[o] = sum_t w4[t] x[2o + t - 1],  x[2q + p] = s2d(x)[p][q]  ->  tap j = q - o + 1, t = 2j + p - 1
    transposed conv   out[2o + p] = sum_q w4[t] x[q], t = 2(o - q) + p + 1           ->  tap j = q - o + 1, t = 3 - 2j + p"""
    A, B = w.shape[:2]
    if standardize:
        w = R._standardize(w)
    kernel = scale.reshape(B, 1, 1, 1, 1) * torch.ones(B, 1, 2, 2, 2, dtype=w.dtype)
    w4 = F.conv3d(w, kernel, padding=1, groups=B)
    wexp = torch.zeros((8 * B, A, 3, 3, 3) if transposed else (A, 8 * B, 3, 3, 3), dtype=w.dtype)
    for p in range(8):
        pz, py, px = p >> 2, (p >> 1) & 1, p & 1
        for jz in range(3):
            for jy in range(3):
                for jx in range(3):
                    tz, ty, tx = ((3 - 2 * j + q) if transposed else (2 * j + q - 1) for j, q in ((jz, pz), (jy, py), (jx, px)))
                    if not (0 <= tz < 4 and 0 <= ty < 4 and 0 <= tx < 4):
                        continue
                    if transposed:
                        wexp[p::8, :, jz, jy, jx] = w4[:, :, tz, ty, tx].t()
                    else:
                        wexp[:, p::8, jz, jy, jx] = w4[:, :, tz, ty, tx]
    return wexp


def _weight_cases():
    cases = []
    for std, tr in ((False, False), (True, True), (True, False), (False, True)):
        A, B = 5, 6
        w = rnd(A, B, 3, 3, 3, seed=1) * 0.3 + 0.05
        scale = torch.full((B,), 0.37) + rnd(B, seed=3) * 0.01

        def oracle(O, t, dys, std=std, tr=tr):
            wexp, ms = O.blur_weight_fwd(t["w"], t["scale"], std, tr)
            return {"out0": wexp, "w": O.blur_weight_bwd(dys[0], t["w"], t["scale"], ms, std, tr)}
        # K:582-587 (test_blur_weight_transform): wexp close(1e-5, 1e-6), dw close(2e-5, 1e-6)
        cases.append(Case(f"blur_weight_std{int(std)}_t{int(tr)}", {"w": w},
                          lambda t, std=std, tr=tr: ops.blur_weight(t["w"], t["scale"], std, tr),
                          lambda t, std=std, tr=tr: _blur_ref(t["w"], t["scale"], std, tr),
                          {"out0": (1e-5, 1e-6), "w": (2e-5, 1e-6)}, consts={"scale": scale}, oracle=oracle))

    def ws_oracle(O, t, dys):
        wn, ms = O.weight_standardize_fwd(t["w"])
        return {"out0": wn, "w": O.weight_standardize_bwd(dys[0], t["w"], ms)}
    # K:594-596 (test_weight_standardize_fwd_bwd): forward close(1e-5, 1e-5), backward close(1e-4, 1e-5)
    for tag, shape in (("ragged", (5, 7, 3, 3, 3)), ("vec", (8, 4, 3, 3, 3))):
        cases.append(Case(f"weight_standardize_{tag}", {"w": rnd(*shape, seed=1)}, lambda t: ops.weight_standardize(t["w"]),
                          lambda t: R._standardize(t["w"]), {"out0": (1e-5, 1e-5), "w": (1e-4, 1e-5)}, oracle=ws_oracle))
    return cases


CASES = CONV + CONVT + NORM + _pool_cases() + _upsample_cases() + _head_cases() + _elementwise_cases() + _weight_cases()
assert len({c.name for c in CASES}) == len(CASES)


# ------------------------------------------------------------------------------------------------- fp64 reference
_REF = {}


def dys_for(case, shapes):
    """the seeded dense upstream gradient of every output"""
    return [rnd(*s, seed=100 + i) if len(s) else torch.tensor(0.7) for i, s in enumerate(shapes)]


def reference(case):
    """fp64 torch on the CPU, once per case: {"outs", "dys" (fp32), "grads", "bounds"}; `bounds` holds the per-element
    bounds of the tolerances given as callables"""
    if case.name not in _REF:
        t = {k: v.double().requires_grad_(True) for k, v in case.inputs.items()}
        t.update({k: (v.double() if v.is_floating_point() else v) for k, v in case.consts.items()})
        outs = _tuple(case.ref(t))
        dys = dys_for(case, [tuple(o.shape) for o in outs])
        grads = torch.autograd.grad(outs, [t[k] for k in case.inputs], [d.double() for d in dys], allow_unused=True)
        t64 = {k: v.detach() for k, v in t.items()}
        bounds = {k: f(t64, [d.double() for d in dys]) for k, f in case.tol.items() if callable(f)}
        _REF[case.name] = dict(outs=[o.detach() for o in outs], dys=dys, grads=dict(zip(case.inputs, grads)), bounds=bounds)
    return _REF[case.name]


def excess(case, key, got, ref, ref_info):
    """|got - ref| as a fraction of what `case.tol[key]` allows (<= 1 passes); for a tolerance of exactly zero: 0.0 when
    equal, inf otherwise.  Against an (rtol, atol) pair the fp64 reference is first rounded ONCE to fp32, the format the
    kernel (and the C oracle these tolerances were set against) stores its result in: several of the pairs -- close(0, 0),
    close(0, 1e-7) -- are below the fp32 resolution of the data, and no fp32 result is closer than half an ulp to an fp64
    value.  The per-element bounds (callables) are stated against the unrounded fp64 value, as the tests they come from do."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (case.name, key, got.shape, ref.shape)
    tol = case.tol[key]
    if not callable(tol):
        ref = ref.float().double()
    err = (got - ref).abs()
    if callable(tol):
        bound = ref_info["bounds"][key]
        bad = err > bound
        if not bool(bad.any()):
            m = bound > 0
            return float((err[m] / bound[m]).max()) if bool(m.any()) else 0.0
        return float("inf") if bool((bound[bad] == 0).any()) else float((err[bad] / bound[bad]).max())
    allowed = tol[1] + tol[0] * ref.abs().max().item()
    worst = err.max().item() if err.numel() else 0.0
    if allowed == 0.0:
        return 0.0 if worst == 0.0 else float("inf")
    return worst / allowed
