"""Tensor-level predictors: the arithmetic of segmentation_pipeline/prediction.py
(reference) without the torchio Subject plumbing.

* split_and_flip / reverse_split_and_flip (:16-27): index-only views.
* StandardPredict.predict (:73-102): optional sagittal split, one model call; the
  prediction stays on the device (the reference's per-subject `.detach().cpu()`, :97,
  is an evaluator concern and forces a sync every iteration).
* PatchPredict.predict (:124-152): torchio GridSampler / GridAggregator('average' or
  'hann') become a deterministic tile list + the patch_gather / patch_aggregate_grid kernels;
  inside `distributed.unit_sharding()` the tiles are sharded over the ranks and
  returned by a single all_gather (distributed.gather_tiles).
"""
import copy
import itertools
from typing import Optional, Sequence, Tuple

import torch

from . import distributed as D
from . import evaluators as E
from . import ops
from . import preprocessing as P
from ._lib import M355Error


def split_and_flip(x: torch.Tensor) -> torch.Tensor:
    first, second = x.split(x.shape[2] // 2, dim=2)
    return torch.cat([first, second.flip(2)], dim=0)


def reverse_split_and_flip(x: torch.Tensor) -> torch.Tensor:
    first, second = x.split(x.shape[0] // 2, dim=0)
    return torch.cat([first, second.flip(2)], dim=2)


def grid_locations(volume_shape, patch_size, patch_overlap):
    """Corner indices of torchio 0.18.45's GridSampler with padding_mode=None (the
    configuration of research/msseg2/msseg2.py:139-146): per axis
    range(0, size - patch + 1, patch - overlap), plus size - patch if the border is not
    reached; patches enumerated in itertools.product order."""
    return [tuple(c) for c in itertools.product(*grid_axes(volume_shape, patch_size, patch_overlap))]


def grid_axes(volume_shape, patch_size, patch_overlap):
    """the per-axis start lists whose product is `grid_locations`"""
    axes = []
    for size, p, o in zip(volume_shape, patch_size, patch_overlap):
        if p > size:
            raise ValueError(f"patch size {p} exceeds volume size {size}")
        if o >= p:
            raise ValueError(f"patch overlap {o} must be smaller than patch size {p}")
        starts = list(range(0, size - p + 1, p - o))
        if starts[-1] != size - p:
            starts.append(size - p)
        axes.append(starts)
    return axes


def _triple(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v, v)


def hann_window_axes(patch_size):
    """The per-axis factors of torchio's GridAggregator('hann') window for `patch_size`: three 1-D fp32 CPU tensors,
    axis x holding torch.hann_window(p + 2, periodic=False)[1:-1] -- p strictly positive values, symmetric, [1.] for
    p = 1.  The weight of voxel (di, dj, dk) of a tile is (w0[di] * w1[dj]) * w2[dk]."""
    return tuple(torch.hann_window(int(p) + 2, periodic=False, dtype=torch.float32)[1:-1].contiguous()
                 for p in _triple(patch_size))


class StandardPredict:
    """Whole-image prediction (reference :57-102), tensors in, tensors out."""

    def __init__(self, image_names: Sequence[str] = ("X",), sagittal_split: bool = False, refine_image: str = None):
        image_names = list(image_names)
        if refine_image is not None and refine_image not in image_names:
            image_names.append(refine_image)
        self.image_names = image_names
        self.sagittal_split = sagittal_split
        self.refine_image = refine_image

    def predict(self, model, device, batch, label_attributes=None):
        """batch: dict of stacked tensors (collate_subjects, utils/utils.py:75-85)."""
        batch = {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in batch.items()}
        x = batch["X"]
        y_pred = model(split_and_flip(x).contiguous()) if self.sagittal_split else model(x)
        if isinstance(y_pred, (tuple, list)):
            # a deep-supervision model in training mode (models.DeepSupervisionUNet): every level for the criterion, the
            # full-resolution one where a tensor is expected (TrainLoop's training evaluators)
            levels = tuple(reverse_split_and_flip(p) for p in y_pred) if self.sagittal_split else tuple(y_pred)
            batch["y_pred_levels"] = levels
            y_pred = levels[0]
        elif self.sagittal_split:
            y_pred = reverse_split_and_flip(y_pred)
        batch["y_pred"] = y_pred
        return batch


class GraphedForward:
    """The no-grad forward of `model` replayed from a hipGraph, one capture per (input shape, precision mode, parameter
    versions).  A sliding window pushes hundreds of same-shaped tile batches through the model (reference :136-141);
    with small patches the forward is launch-bound -- ~80 launches of a few microseconds of GPU work each against
    1.3-2 ms of host enqueue time -- and a replay is one launch.  Capture is safe here because every launch of the
    library goes to the current stream, the work queues are reset on the device, workspaces come from torch's
    allocator (the graph's private pool) and the packed-weight caches are filled by the warm-up passes; the result
    is bit-identical to the eager forward (`tools/graph_probe.py`, tests).  The output tensor is owned by the graph:
    it is valid until the next call with the same key (callers that keep it, as PatchPredict does, get a copy).
    Large patches are GPU-bound and gain nothing (cfg4: 2.14 ms eager vs 2.21 ms replayed in bf16)."""

    def __init__(self, model, copy_output: bool = True, max_graphs: int = 4):
        self.model, self.copy_output, self.max_graphs = model, copy_output, max_graphs
        self._graphs = {}

    def _key(self, x):
        # storage AND version of every parameter / buffer: a replaced Parameter, `module.to()` or an optimizer step
        # all invalidate the capture (a sum of versions alone would replay a graph that reads freed storage).
        # In-place writes through `.data` bump no version and are not supported on a captured model.
        version = hash(tuple((t.data_ptr(), t._version) for t in
                             itertools.chain(self.model.parameters(), self.model.buffers())))
        return (tuple(x.shape), x.dtype, x.device, ops.get_precision(), self.model.training, version)

    def __call__(self, x):
        if not x.is_cuda:
            return self.model(x)
        key = self._key(x)
        ent = self._graphs.get(key)
        if ent is None:
            if len(self._graphs) >= self.max_graphs:     # (a new parameter version or shape: drop the oldest capture)
                self._graphs.pop(next(iter(self._graphs)))
            static_x = x.clone()
            side = torch.cuda.Stream(device=x.device)
            side.wait_stream(torch.cuda.current_stream(x.device))
            with torch.cuda.stream(side), torch.no_grad():
                for _ in range(2):                        # warm-up: allocator, packed weights, derived filters
                    self.model(static_x)
            torch.cuda.current_stream(x.device).wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph), torch.no_grad():
                static_y = self.model(static_x)
            ent = self._graphs[key] = (graph, static_x, static_y)
        graph, static_x, static_y = ent
        static_x.copy_(x)
        graph.replay()
        return static_y.clone() if self.copy_output else static_y


class PatchPredict:
    """Sliding-window prediction with overlap averaging (reference :105-152).

    overlap_mode (reference :115,134 -> torchio GridAggregator): 'average' (every covering tile has the same vote) or
    'hann' (each tile is weighted by a Hann window that fades towards its faces, `hann_window_axes`, and the sum is
    divided by the summed weights: no seams at tile borders).  'hann' needs a backend with `patch_aggregate_grid`;
    'crop' is not implemented.

    padding_mode (reference :114,132 -> torchio GridSampler): None, a number (constant fill) or one of numpy.pad's
    'constant' / 'edge' / 'reflect' / 'symmetric' / 'wrap': the volume is treated as padded by patch_overlap // 2
    voxels per side before tiling, and the aggregate is cropped back (index math in the gather / finalize
    kernels; no padded copy).  The other numpy.pad modes (statistics, ramps) have no kernel.

    Multi-GPU (inside `distributed.unit_sharding()`): tile i -> rank i % world, one collective returns the tile
    outputs.  `result_on="all"` (default): all_gather, every rank aggregates and returns the volume;
    `result_on="rank0"`: gather to rank 0 only, which alone aggregates (the other ranks return None) -- no rank
    receives or re-aggregates tiles it does not need.  `timings` (a dict) accumulates seconds per phase
    (tile_gather, model, exchange, accumulate, finalize; a device synchronisation per stamp, for profiling).
    `graph=True`: full tile batches go through a `GraphedForward` of the model (launch-bound small patches).
    """

    def __init__(self, image_names: Sequence[str] = ("X",), patch_batch_size: int = 16, patch_size=None,
                 patch_overlap=(0, 0, 0), padding_mode=None, overlap_mode: str = "average", ops_backend=ops,
                 result_on: str = "all", timings: Optional[dict] = None, graph: bool = False):
        if overlap_mode not in ("average", "hann"):
            raise NotImplementedError("only overlap_mode='average' (the mode the reference uses) and 'hann' are implemented")
        if overlap_mode != "average" and not hasattr(ops_backend, "patch_aggregate_grid"):
            raise NotImplementedError(f"overlap_mode={overlap_mode!r} needs an ops backend with patch_aggregate_grid: the "
                                      "accumulate / finalize fallback serves 'average' only")
        self.pad_value = 0.0
        if padding_mode is not None and not isinstance(padding_mode, str):
            self.pad_value, padding_mode = float(padding_mode), "constant"
        if padding_mode is not None and padding_mode not in ops.PAD_MODES:
            raise NotImplementedError(f"padding_mode={padding_mode!r} has no kernel (supported: None, a number, "
                                      f"{sorted(ops.PAD_MODES)})")
        if result_on not in ("all", "rank0"):
            raise ValueError("result_on must be 'all' or 'rank0'")
        self.image_names = image_names
        self.patch_batch_size = patch_batch_size
        self.patch_size = _triple(patch_size)
        self.patch_overlap = _triple(patch_overlap)
        self.padding_mode = padding_mode
        self.overlap_mode = overlap_mode
        self.result_on = result_on
        self.timings = timings
        self.graph = graph
        self._graphed = None     # (model, GraphedForward)
        self._window = None      # (patch size, hann_window_axes of it)
        self._ops = ops_backend  # the HIP ops; tests inject a CPU double for the gloo plumbing test

    def _stamp(self, name, t0, device):
        if self.timings is None:
            return t0
        import time
        if device.type == "cuda":
            torch.cuda.synchronize(device)
        now = time.perf_counter()
        self.timings[name] = self.timings.get(name, 0.0) + (now - t0)
        return now

    def _hann_window(self):
        if self._window is None or self._window[0] != self.patch_size:
            self._window = (self.patch_size, hann_window_axes(self.patch_size))
        return self._window[1]

    def predict_volume(self, model, volume: torch.Tensor) -> Optional[torch.Tensor]:
        """volume [C, V0, V1, V2] on the device -> averaged prediction [C_out, V0, V1, V2]."""
        import time
        k = self._ops
        vshape = tuple(volume.shape[1:])
        border = tuple(o // 2 for o in self.patch_overlap) if self.padding_mode is not None else (0, 0, 0)
        pshape = tuple(v + 2 * b for v, b in zip(vshape, border))        # the (virtually) padded volume
        locs = grid_locations(pshape, self.patch_size, self.patch_overlap)
        dev = volume.device
        run = model
        if self.graph and dev.type == "cuda":
            if self._graphed is None or self._graphed[0] is not model:
                self._graphed = (model, GraphedForward(model, copy_output=False))
            run = self._graphed[1]
        t = time.perf_counter()
        with D.shard_scope() as sharded:  # tiles over ranks only inside distributed.unit_sharding(), outermost sharder
            world = torch.distributed.get_world_size() if sharded else 1
            rank = torch.distributed.get_rank() if sharded else 0
            mine = D.shard_indices(len(locs), rank, world)
            outs = []
            with torch.no_grad():
                for s in range(0, len(mine), self.patch_batch_size):
                    idx = mine[s:s + self.patch_batch_size]
                    loc = torch.tensor([locs[i] for i in idx], dtype=torch.int32, device=dev)
                    if self.padding_mode is None:
                        tiles_in = k.patch_gather(volume, loc, self.patch_size)
                    else:
                        tiles_in = k.patch_gather_padded(volume, loc, self.patch_size, border, self.padding_mode,
                                                         self.pad_value)
                    t = self._stamp("tile_gather", t, dev)
                    # (the graph's output buffer is reused by the next replay: torch.cat below copies, but only after
                    # the loop, so a graphed batch is cloned here; the ragged last batch is a second capture, keyed by
                    # its shape -- it recurs once per volume)
                    outs.append(run(tiles_in).clone() if run is not model else model(tiles_in))
                    t = self._stamp("model", t, dev)
        local = torch.cat(outs, dim=0) if outs else None
        meta = torch.tensor([local.shape[1] if local is not None else 0], device=dev)
        if world > 1:  # ranks without tiles learn the channel count (tiny, once per volume)
            torch.distributed.all_reduce(meta, op=torch.distributed.ReduceOp.MAX)
        c_out = int(meta.item())
        to_rank0 = world > 1 and self.result_on == "rank0"
        tiles = D.gather_tiles(local, len(locs), (c_out,) + self.patch_size, torch.float32, dev, sharded=world > 1,
                               dst=0 if to_rank0 else None)
        t = self._stamp("exchange", t, dev)
        if tiles is None:       # result_on="rank0" and this is another rank
            return None
        # aggregation in grid order: identical bits regardless of world size.  One pass over the tile grid (per voxel:
        # the covering tiles summed in tile order, divided by their count) where the backend has it -- no accumulator /
        # count volumes, no zero-fill, no read-modify-write; the same bits as the batch-by-batch loop below.
        if hasattr(k, "patch_aggregate_grid"):
            axes = grid_axes(pshape, self.patch_size, self.patch_overlap)
            if self.overlap_mode == "hann":
                out = k.patch_aggregate_grid(tiles, axes, vshape, border, window=self._hann_window())
            else:
                out = k.patch_aggregate_grid(tiles, axes, vshape, border)
            self._stamp("aggregate", t, dev)
            return out
        # (backends without it: the batch-by-batch accumulate / finalize, 'average' only -- see the constructor)
        accum = torch.zeros((c_out,) + pshape, dtype=torch.float32, device=dev)
        count = torch.zeros(pshape, dtype=torch.float32, device=dev)
        all_loc = torch.tensor(locs, dtype=torch.int32, device=dev)
        for s in range(0, len(locs), self.patch_batch_size):  # same batching as the reference loop (:136-141)
            k.patch_accumulate(tiles[s:s + self.patch_batch_size], all_loc[s:s + self.patch_batch_size], accum, count)
        t = self._stamp("accumulate", t, dev)
        out = k.patch_finalize(accum, count) if self.padding_mode is None else k.patch_finalize_crop(accum, count, border)
        self._stamp("finalize", t, dev)
        return out

    def predict(self, model, device, batch, label_attributes=None):
        x = batch["X"].to(device)
        batch = dict(batch)
        preds = [self.predict_volume(model, v) for v in x]
        batch["y_pred"] = None if any(p is None for p in preds) else torch.stack(preds)
        return batch


# ---------------------------------------------------------------------------------------------- evaluation labels
class EvaluationPlan:
    """The inverse of a preprocessing chain's label transforms (the reference's
    `filter_transform(history, [LabelTransform, CopyProperty, RenameProperty, ConcatenateImages]).inverse()`,
    prediction.py:155-170) for the image `name`, as a channel -> label value table: CustomOneHot^-1 is the argmax,
    CustomRemapLabels^-1 the swapped remap under the same mask (named remaps restore their label_values entries),
    renames follow the name back.  Built once per chain; `tables(C)` gives the [outside, inside] tables of C channels."""

    def __init__(self, transform, name="y"):
        steps = _label_steps(transform)
        self.final_name = name
        self.remaps = []            # (mapping, named pairs or None, masked) in application order
        self.half, self.mask_name = None, None
        masking = None
        argmax = False
        cur = name
        for t, include, exclude in reversed(steps):
            applies = (include is None or cur in include) and cur not in exclude
            if isinstance(t, P.CustomOneHot):
                if applies:
                    if argmax:
                        raise M355Error("evaluation labels: two CustomOneHot transforms act on one label map")
                    argmax = True
            elif isinstance(t, P.RenameProperty):
                if cur == t.new_name:
                    cur = t.old_name
            elif isinstance(t, P.ConcatenateImages):
                if cur == t.new_image_name:
                    raise M355Error(f"evaluation labels: {cur} is a concatenation; splitting it is not supported")
            elif isinstance(t, P.CustomRemapLabels):
                if not applies:
                    continue
                if not argmax:
                    raise M355Error("evaluation labels: a CustomRemapLabels after CustomOneHot cannot be inverted on "
                                    "label values")
                if not t.invertible:
                    raise M355Error("evaluation labels: a CustomRemapLabels with invertible=False")
                inverse = {}
                for old, new in t.mapping.items():
                    inverse[new] = old
                named = None if t.named is None else [(label, new, old) for label, old, new in t.named]
                if named is not None:
                    inverse = {}
                    for _, new, old in named:
                        inverse[new] = old
                mm = t.masking_method
                if mm is not None:
                    if masking is not None and masking != mm:
                        raise M355Error(f"evaluation labels: remaps under two masks ({masking!r}, {mm!r})")
                    masking = mm
                self.remaps.append((inverse, named, mm is not None))
        if not argmax:
            raise M355Error(f"evaluation labels: no CustomOneHot produced {name}; nothing to take the argmax of")
        self.source_name = cur
        if masking is not None:
            if isinstance(masking, str) and masking.title() in P._ANATOMICAL:
                self.half = P._ANATOMICAL[masking.title()]
            elif isinstance(masking, str):
                self.mask_name = masking
            else:
                raise M355Error(f"evaluation labels: masking_method {masking!r}")

    def tables(self, C):
        outside, inside = list(range(C)), list(range(C))
        for mapping, _, masked in self.remaps:
            inside = [mapping.get(v, v) for v in inside]
            if not masked:
                outside = [mapping.get(v, v) for v in outside]
        return outside, inside

    def label_values(self, label_values):
        """the label_values after the inverse chain (named remaps restore their entries)"""
        if label_values is None:
            return None
        out = copy.deepcopy(dict(label_values))
        for _, named, _ in self.remaps:
            for label, _, old in named or ():
                out[label] = old
        return out


def _label_steps(transform, include=None, exclude=(), gated=False):
    """(label transform, effective include, effective exclude) in the order a Compose runs them; a label transform
    under a probability below 1 or inside OneOf is refused"""
    from . import augmentation as A
    label_types = (P.CustomRemapLabels, P.CustomOneHot, P.RenameProperty, P.ConcatenateImages)
    inc = transform.include if include is None else (
        include if transform.include is None else [k for k in transform.include if k in include])
    exc = list(exclude) + list(transform.exclude)
    gated = gated or transform.probability < 1.0 or isinstance(transform, A.OneOf)
    if isinstance(transform, A.Compose):
        out = []
        for t in transform.transforms:
            out += _label_steps(t, inc, exc, gated)
        return out
    if isinstance(transform, label_types):
        if gated:
            raise M355Error(f"evaluation labels: {type(transform).__name__} runs under a probability gate or inside "
                            "OneOf; its inverse is not defined")
        return [(transform, inc, exc)]
    return []


class _ScoreSource:
    def __init__(self, plan, scores, target, mask, label_values):
        self.plan, self.scores, self.target, self.mask = plan, scores, target, mask
        self.pred_map = E.ScoreLabelMap(self, "pred", label_values)
        self.target_map = None if target is None else E.ScoreLabelMap(self, "target", label_values)

    def materialise(self):
        _materialise([self])


def _materialise(sources):
    plan = sources[0].plan
    has_t = [s.target is not None for s in sources]
    C = sources[0].scores.shape[0]
    outside, inside = plan.tables(C)
    _, preds, targets = ops.eval_scores(
        [s.scores for s in sources], (outside, inside), [outside[0]],
        targets=[s.target for s in sources] if all(has_t) else None,
        masks=[s.mask for s in sources] if plan.mask_name is not None else None, half=plan.half,
        write_pred=True, write_target=all(has_t))
    for i, s in enumerate(sources):
        s.pred_map['data'] = preds[i]
        if s.target_map is not None:
            if targets is None:
                _materialise_one_target(s)
            else:
                s.target_map['data'] = targets[i]


def _materialise_one_target(s):
    outside, inside = s.plan.tables(s.scores.shape[0])
    _, _, targets = ops.eval_scores([s.target.to(torch.float32)], (outside, inside), [outside[0]], targets=[s.target],
                                    masks=[s.mask] if s.plan.mask_name is not None else None, half=s.plan.half,
                                    write_target=True)
    s.target_map['data'] = targets[0]


def _tensor(v):
    return v if torch.is_tensor(v) else v.data


def split_batch(batch, pred_name="y_pred", target_name="y"):
    """One batch dict of stacked [N, C, D, H, W] tensors (optionally 'name': a list) as a list of N subject dicts: the
    scores, the target and every other 5-D tensor are indexed (views), anything else is shared."""
    n = next(_tensor(v).shape[0] for k, v in batch.items() if k in (pred_name, target_name))
    names = batch.get("name", [None] * n)
    return [{k: (_tensor(v)[i] if k in (pred_name, target_name) or
                 (torch.is_tensor(v) and v.dim() == 5) else v)
             for k, v in batch.items() if k != "name"} | ({"name": names[i]} if names[i] is not None else {})
            for i in range(n)]


def add_evaluation_labels(subjects, transform, label_values=None, write=False, pred_name="y_pred", target_name="y"):
    """Add 'y_pred_eval' / 'y_eval' label maps (evaluators.LabelMap: int64 [1, D, H, W] and 'label_values') to every
    subject that has 'y_pred' scores ([C, D, H, W]) or a one-hot 'y', inverting the label transforms of `transform`,
    the preprocessing Compose that produced 'y' (prediction.py:155-170 of the reference).  `label_values`: the training
    target's {label name: value} after the chain (the reference's label_attributes); both maps take its inverse.
    `subjects`: a list of dicts, or one batch dict of stacked [N, C, D, H, W] tensors (optionally 'name': a list),
    which becomes a list of subject dicts.  The maps are computed on first access to `.data`; an evaluator counts
    straight from the scores without writing them.  write=True: compute them now, in one launch.
    A masked remap whose mask is a label map reads it from the subject under its name.  Returns the subjects."""
    if isinstance(subjects, dict):
        subjects = split_batch(subjects, pred_name, target_name)
    plan = transform if isinstance(transform, EvaluationPlan) else EvaluationPlan(transform, target_name)
    values = plan.label_values(label_values)
    sources = []
    for s in subjects:
        scores = _tensor(s[pred_name]) if pred_name in s else None
        target = _tensor(s[target_name]) if target_name in s else None
        mask = None
        if plan.mask_name is not None:
            if plan.mask_name not in s:
                raise M355Error(f"evaluation labels: the remap mask {plan.mask_name} is not in the subject")
            mask = _tensor(s[plan.mask_name])
        if scores is None and target is None:
            continue
        if scores is None:   # a target alone: the table applies to its argmax
            src = _ScoreSource(plan, target.to(torch.float32), None, mask, values)
            s["y_eval"] = src.pred_map
            continue
        src = _ScoreSource(plan, scores, target, mask, values)
        s["y_pred_eval"] = src.pred_map
        if src.target_map is not None:
            s["y_eval"] = src.target_map
        sources.append(src)
    if write and sources:
        _materialise(sources)
    return subjects
