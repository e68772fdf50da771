"""Dataset fingerprint (data_processing/dataset_fingerprint.py, reference): per subject the spacing, the spatial shape,
the bounding box of every label and mean / std / median / min / max of every image, then the same five statistics of
each of these numbers over the subjects.  It is what one looks at before choosing CropOrPad targets, patch sizes and
TargetResample(target_spacing="median") (preprocessing.py).

The volumes stay on the device: a subject costs one ops.region_stats call (csrc/region_stats.hip) -- the
bounds of all its label maps and the whole-volume statistics of all its images -- and one copy of a few hundred bytes
back.  The summary over the subjects is host arithmetic on short lists, in torch like the reference's, so it gives the
reference's numbers for the same per-subject values.

Subjects are mappings with a 'name'; their images are told apart by class: evaluators.ScalarImage and
evaluators.LabelMap (a label map carries 'label_values': {label name: value}).  `spacing` and `spatial_shape` are read
from the subject (attribute or key) when it has them, else from its first image (spacing 1 when nothing says).
"""
import copy
import json
from pathlib import Path
from typing import Optional, Sequence

import torch

from .. import ops
from ..evaluators import LabelMap, ScalarImage, _device_tensors, _image_spacing

__all__ = ["get_bounds", "get_label_bounds", "get_summary_stats", "merge_dict", "summarize", "get_dataset_fingerprint"]

STATS = ops.REGION_STATS


def _bounds_entry(bounds6, shape, what):
    """the reference's four views of a bounding box (get_bounds), its conventions kept: `crop` pairs the first index
    with shape - last index (one more than the voxels after the box), `size` is last - first (one less than the voxels
    spanned), `center` their midpoint"""
    lo, hi = [int(v) for v in bounds6[0::2]], [int(v) for v in bounds6[1::2]]
    if any(h < l for l, h in zip(lo, hi)):
        raise ValueError(f"{what} has no voxel: an empty mask has no bounds")
    out = {"extents": [], "crop": [], "size": [], "center": []}
    for l, h, n in zip(lo, hi, shape):
        out["extents"] += [l, h]
        out["crop"] += [l, int(n) - h]
        out["size"].append(h - l)
        out["center"].append((h + l) / 2)
    return out


def _volume(data):
    """[W, H, D] of a label map's data ([1, W, H, D] or [W, H, D])"""
    if data.dim() == 4 and data.shape[0] == 1:
        return data[0]
    if data.dim() != 3:
        raise ValueError(f"expected a volume [W, H, D] or [1, W, H, D], got shape {tuple(data.shape)}")
    return data


def get_bounds(mask: torch.Tensor):
    """{'extents', 'crop', 'size', 'center'} of the nonzero voxels of a volume [W, H, D]; ValueError when there is none"""
    vol, = _device_tensors([_volume(mask)])
    res = ops.region_stats(vol, [], [])
    return _bounds_entry(res.bounds[0].cpu().tolist(), vol.shape, "the mask")


def _label_bounds(bounds, label_values, shape, name):
    """rows of RegionStats.bounds (the listed values, then 'all') -> the reference's dict, 'all' first"""
    names = list(label_values)
    out = {"all": _bounds_entry(bounds[len(names)], shape, f"{name}: the foreground")}
    for i, label_name in enumerate(names):
        out[label_name] = _bounds_entry(bounds[i], shape, f"{name}: label {label_name!r} ({label_values[label_name]})")
    return out


def get_label_bounds(label_map):
    """{'all': bounds of `data != 0`, label name: bounds of `data == value` ...} of a label map with 'label_values'"""
    label_values = label_map['label_values']
    vol, = _device_tensors([_volume(label_map.data)])
    res = ops.region_stats(vol, [], [int(v) for v in label_values.values()])
    return _label_bounds(res.bounds.cpu().tolist(), label_values, vol.shape, "label map")


def _plain(x):
    """a tensor, or the `.values` of a (values, indices) result, as a number or a tuple of numbers"""
    x = x if isinstance(x, torch.Tensor) else x.values
    return x.item() if x.numel() == 1 else tuple(x.tolist())


def get_summary_stats(tensor: torch.Tensor, **kwargs):
    """{'mean', 'std', 'median', 'min', 'max'} of a tensor.  A device tensor without keyword arguments goes through
    ops.region_stats (all elements pooled, float32 results).  Anything else is torch on the host, `kwargs` (e.g.
    dim=0) handed to every function: mean and unbiased std of the values as float32, median (lower middle), min and
    max in the tensor's own type; results along a dimension come back as tuples."""
    if tensor.is_cuda and not kwargs:
        x = tensor if tensor.dim() == 4 else tensor.reshape(1, 1, 1, -1)
        row = ops.region_stats(torch.zeros(x.shape[1:], dtype=torch.uint8, device=x.device), [x], []).stats[1, 0]
        return dict(zip(STATS, row.cpu().tolist()))
    as_float = tensor.float()
    return {'mean': _plain(torch.mean(as_float, **kwargs)), 'std': _plain(torch.std(as_float, **kwargs)),
            'median': _plain(torch.median(tensor, **kwargs)), 'min': _plain(torch.min(tensor, **kwargs)),
            'max': _plain(torch.max(tensor, **kwargs))}


def merge_dict(in_dict: dict, out_dict: dict):
    """append every leaf of in_dict to the list at the same place of out_dict (created on first sight): merging the
    subjects' fingerprints one by one turns each leaf into the list of its values over the subjects"""
    for key, value in in_dict.items():
        if isinstance(value, dict):
            merge_dict(value, out_dict.setdefault(key, {}))
        else:
            out_dict.setdefault(key, []).append(value)


def summarize(elem):
    """the five statistics over the subjects (dim 0) of every list of a merged fingerprint, the nesting kept"""
    if isinstance(elem, dict):
        return {key: summarize(value) for key, value in elem.items()}
    if isinstance(elem, list):
        return get_summary_stats(torch.tensor(elem), dim=0)
    raise RuntimeError(f"Unexpected element {elem}")


def _subject_property(subject, name):
    value = getattr(subject, name, None)
    if value is None and name in subject:
        value = subject[name]
    return value


def _fingerprint(subject, image_names):
    if image_names is None:
        names = list(subject.keys())
    else:
        names = [name for name in image_names if name in subject]
    images = {name: subject[name] for name in names if isinstance(subject[name], ScalarImage)}
    label_maps = {name: subject[name] for name in names if isinstance(subject[name], LabelMap)}
    every = list(label_maps.values()) + list(images.values())

    spacing = _subject_property(subject, 'spacing')
    if spacing is None:
        spacing = _image_spacing(every[0], None) if every else (1.0, 1.0, 1.0)
    shape = _subject_property(subject, 'spatial_shape')
    if shape is None and every:
        shape = tuple(every[0].data.shape[-3:])
    fingerprint = {'spacing': tuple(spacing), 'spatial_shape': None if shape is None else tuple(int(v) for v in shape),
                   'label_bounds': {}, 'intensity_stats': {}}
    if not every:
        return fingerprint

    # one call: entry m is label map m with its own values; the images ride with the first entry (without a label
    # map, with a blank one), whose 'whole' row is their unmasked statistics
    tensors = _device_tensors([_volume(m.data) for m in label_maps.values()] + [im.data for im in images.values()])
    vols, ims = tensors[:len(label_maps)], tensors[len(label_maps):]
    values = [[int(v) for v in m['label_values'].values()] for m in label_maps.values()]
    if not vols:
        vols, values = [torch.zeros(ims[0].shape[-3:], dtype=torch.uint8, device=ims[0].device)], [[]]
    res = ops.region_stats(vols, [ims] + [[] for _ in vols[1:]], values)
    for m, (name, label_map) in enumerate(label_maps.items()):
        fingerprint['label_bounds'][name] = _label_bounds(res[m].bounds.tolist(), label_map['label_values'],
                                                          vols[m].shape, f"{subject['name']}: {name}")
    whole = res[0].stats[-1]
    for k, name in enumerate(images):
        fingerprint['intensity_stats'][name] = dict(zip(STATS, whole[k].tolist()))
    return fingerprint


def get_dataset_fingerprint(dataset, transform=None, save: bool = False, image_names: Optional[Sequence[str]] = None):
    """-> (subject_fingerprints {subject name: fingerprint}, summary_fingerprint).  A fingerprint is
    {'spacing', 'spatial_shape', 'label_bounds': {label map: {'all' | label name: {'extents', 'crop', 'size',
    'center'}}}, 'intensity_stats': {image: {'mean', 'std', 'median', 'min', 'max'}}}; the summary has the same nesting
    with every leaf replaced by its five statistics over the subjects.

    dataset: an object with `.all_subjects` (and `.root` for save=True), or a sequence of subjects.  transform: a
    callable subject -> subject applied to a deep copy of every subject first (a device preprocessing chain, wrapped to
    take and return a subject).  image_names: only these images and label maps.  save=True writes
    <root>/fingerprint/subject_fingerprints.json and fingerprint.json.  A label of 'label_values' that a subject does
    not contain raises ValueError, as an empty mask has no bounds."""
    subjects = dataset.all_subjects if hasattr(dataset, 'all_subjects') else dataset
    subject_fingerprints = {}
    for subject in subjects:
        if transform is not None:
            subject = copy.deepcopy(subject)
            if hasattr(subject, 'load'):
                subject.load()
            subject = transform(subject)
        subject_fingerprints[subject['name']] = _fingerprint(subject, image_names)

    merged = {}
    for fingerprint in subject_fingerprints.values():
        merge_dict(fingerprint, merged)
    summary_fingerprint = summarize(merged)

    if save:
        out_path = Path(dataset.root) / "fingerprint"
        out_path.mkdir(parents=True, exist_ok=True)
        with (out_path / "subject_fingerprints.json").open("w") as f:
            json.dump(subject_fingerprints, f, indent=2)
        with (out_path / "fingerprint.json").open("w") as f:
            json.dump(summary_fingerprint, f, indent=2)
    return subject_fingerprints, summary_fingerprint
