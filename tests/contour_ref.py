"""CPU restatement of the contour images for the tests: per-slice foreground counts and their ranking in torch, slicing
and make_grid in numpy, and the reference's drawing calls.  Written from the description of the reference's behaviour
(transforms/find_interesting_slice.py, utils.slice_volume, torchvision.utils.make_grid with padding 1,
evaluators/contour_image_evaluator.py); tests/test_contour_cpu.py ties it to the reference's recorded results
(tests/golden/contour.npz)."""
import io
import random
import warnings

import numpy as np
import torch

PLANES = ("Saggital", "Coronal", "Axial")


def foreground(data, one_hot=False):
    """bool [W, H, D] of a holder's data [C, W, H, D]"""
    data = data.cpu()
    if one_hot:
        return torch.argmax(data.float(), dim=0) != 0
    return data[0] != 0


def slice_counts(mask):
    """int64 counts per sagittal, coronal and axial slice of a bool [W, H, D]"""
    m = mask.to(torch.int64)
    return [m.sum(dim=(1, 2)), m.sum(dim=(0, 2)), m.sum(dim=(0, 1))]


def rank(counts):
    """(slice ids with a non-zero count by count descending, ties by ascending id; their counts)"""
    counts = counts.tolist()
    ids = sorted((k for k, c in enumerate(counts) if c > 0), key=lambda k: (-counts[k], k))
    return ids, [counts[k] for k in ids]


def interesting(data, one_hot=False):
    """({plane: ids}, {plane: counts}) as lists"""
    ranked = [rank(c) for c in slice_counts(foreground(data, one_hot))]
    return {p: r[0] for p, r in zip(PLANES, ranked)}, {p: r[1] for p, r in zip(PLANES, ranked)}


def slice_property(size3, ranked, slice_id, plane):
    """the entry at rank slice_id; the last one past the end; the middle of the axis when nothing is ranked"""
    values = ranked[plane]
    if not values:
        return size3[PLANES.index(plane)] // 2
    return values[min(slice_id, len(values) - 1)]


def slice_volume(x, plane, k):
    """x: numpy [W, H, D] -> the 2-D slice"""
    if plane == "Axial":
        return x[:, :, k]
    if plane == "Coronal":
        return np.rot90(x[:, k, :])
    if plane == "Saggital":
        return np.rot90(x[k, :, :])
    raise ValueError(plane)


def make_grid(tiles, ncol, pad_value):
    """numpy tiles of one shape -> the grid (a single tile comes back bare)"""
    n = len(tiles)
    if n == 1:
        return np.array(tiles[0])
    h, w = tiles[0].shape
    xmaps = min(ncol, n)
    ymaps = (n + xmaps - 1) // xmaps
    grid = np.full((ymaps * (h + 1) + 1, xmaps * (w + 1) + 1), pad_value, dtype=tiles[0].dtype)
    for k, t in enumerate(tiles):
        r, c = (k // xmaps) * (h + 1) + 1, (k % xmaps) * (w + 1) + 1
        grid[r:r + h, c:c + w] = t
    return grid


def to_numpy(t):
    t = t.cpu()
    return t.float().numpy() if t.dtype in (torch.bfloat16, torch.float16) else t.numpy()


def mosaic(subjects, name, resolved, ncol, pad_value, impute_shape, dtype=None):
    """subjects: dicts of holders with `.data` [C, W, H, D]; resolved: [(slice id, plane)] per subject"""
    present = [to_numpy(s[name].data[0]) for s in subjects if name in s]
    dtype = dtype or (present[0].dtype if present else np.float32)
    tiles = []
    for s, (k, plane) in zip(subjects, resolved):
        if name in s:
            tiles.append(slice_volume(to_numpy(s[name].data[0]), plane, k))
        else:
            tiles.append(np.zeros(impute_shape, dtype))
    return make_grid(tiles, ncol, pad_value)


def resolve(subjects, plane, slice_id, interesting_slice, target_name, pred_name):
    """[(slice id, plane)] per subject and the plane in use; `plane` already drawn when it was 'random'"""
    if not interesting_slice:
        return [(slice_id, plane)] * len(subjects)
    out = []
    for s in subjects:
        holder = s[target_name] if target_name in s else s[pred_name]
        size3 = tuple(holder.data.shape[1:])
        ids, counts = interesting(holder.data, bool(holder.get("one_hot", False)))
        if plane.lower() == "interesting":
            best = -1
            for p in ("Axial", "Coronal", "Saggital"):
                c = slice_property(size3, counts, slice_id, p)
                if c > best:
                    plane, best = p, c
        out.append((slice_property(size3, ids, slice_id, plane), plane))
    return out


def slice_shape(size3, plane):
    W, H, D = size3
    return {"Axial": (W, H), "Coronal": (D, W), "Saggital": (D, H)}[plane]


def mosaics(subjects, plane, image_name, pred_name, target_name, slice_id, ncol, interesting_slice=False):
    """(resolved, image mosaic, target mosaic or None, prediction mosaic or None, label_values) of one get_image call"""
    out_pred = pred_name is not None and pred_name in subjects[0]
    out_target = target_name is not None and target_name in subjects[0]
    label_values = {}
    if out_pred:
        label_values = subjects[0][pred_name]["label_values"]
    if out_target:
        label_values = subjects[0][target_name]["label_values"]
    if plane.lower() == "random":
        plane = ("Axial", "Coronal", "Saggital")[random.randint(0, 2)]
    resolved = resolve(subjects, plane, slice_id, interesting_slice, target_name, pred_name)
    plane = resolved[0][1]
    resolved = [(k, plane) for k, _ in resolved]
    shape = slice_shape(tuple(subjects[0][image_name].data.shape[1:]), plane)
    img = mosaic(subjects, image_name, resolved, ncol, -1, shape)
    y = mosaic(subjects, target_name, resolved, ncol, 0, shape) if out_target else None
    y_pred = mosaic(subjects, pred_name, resolved, ncol, 0, shape) if out_pred else None
    return resolved, img, y, y_pred, label_values


def render(img, y, y_pred, label_values, scale=0.1, line_width=1.5, legend=False):
    """the picture: the image in gray, target labels contoured at 0.5 solid, prediction labels at 0.95 dashed, colours
    by label id, saved tight on black into a PIL.Image"""
    import matplotlib
    import matplotlib.pyplot as plt
    from PIL import Image
    H, W = img.shape
    fig = plt.figure(figsize=(W * scale, H * scale))
    plt.imshow(img, cmap="gray")
    X, Y = np.meshgrid(np.linspace(0, W - 1, W), np.linspace(0, H - 1, H))
    colours = [None, "r", "g", "b", "y", "c", "m"]
    for name in ("Accent", "Dark2", "Set1", "Set2", "tab20"):
        colours += list(matplotlib.colormaps[name].colors)
    drawn = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if y is not None:
            for label_name, v in label_values.items():
                drawn.append(plt.contour(X, Y, y == v, levels=[0.5], colors=colours[v:v + 1], linewidths=line_width,
                                         alpha=1.))
                if legend:
                    plt.legend([c.legend_elements()[0][0] for c in drawn], label_values.items(), ncol=3,
                               bbox_to_anchor=(0.5, 0), loc="upper center", fancybox=True)
        if y_pred is not None:
            for label_name, v in label_values.items():
                plt.contour(X, Y, y_pred == v, levels=[0.95], linestyles="dashed", colors=colours[v:v + 1],
                            linewidths=line_width, alpha=1.)
    plt.tick_params(which="both", bottom=False, top=False, left=False, labelbottom=False, labelleft=False)
    buf = io.BytesIO()
    fig.savefig(buf, bbox_inches="tight", pad_inches=0.0, facecolor="black")
    buf.seek(0)
    image = Image.open(buf)
    image.load()
    plt.close(fig)
    return image
