"""Host float64 restatement of the device augmentation (segmentation_pipeline_amd.augmentation) in numpy /
scipy: what the GPU tests replay each call's `last_history` against."""
import numpy as np

_M32 = np.uint64(0xFFFFFFFF)


# ------------------------------------------------------------------------------------------------ spatial
def bspline_weights(f):
    f = np.asarray(f, dtype=np.float64)
    g = 1.0 - f
    return np.stack([g ** 3 / 6, (3 * f ** 3 - 6 * f ** 2 + 4) / 6, (-3 * f ** 3 + 3 * f ** 2 + 3 * f + 1) / 6, f ** 3 / 6])


def mirror(i, n):
    if n == 1:
        return np.zeros_like(i)
    period = 2 * n - 2
    i = np.abs(i) % period
    return np.where(i >= n, period - i, i)


def prefilter(x):
    """cubic B-spline coefficients of every channel (scipy spline_filter, order 3, mode 'mirror')"""
    import scipy.ndimage as ndi
    return np.stack([ndi.spline_filter(c.astype(np.float64), order=3, mode="mirror") for c in x])


def displacement(grid, out_shape):
    """cubic B-spline displacement [3, *out_shape] of a control grid [K0, K1, K2, 3] spanning the volume"""
    K = grid.shape[:3]
    ws, bases = [], []
    for a in range(3):
        u = (np.arange(out_shape[a]) + 0.5) * ((K[a] - 3) / out_shape[a])
        b = np.clip(np.floor(u).astype(np.int64), 0, K[a] - 4)
        ws.append(bspline_weights(u - b))
        bases.append(b)
    d = np.zeros((3,) + tuple(out_shape))
    for i in range(4):
        for j in range(4):
            for k in range(4):
                w = ws[0][i][:, None, None] * ws[1][j][None, :, None] * ws[2][k][None, None, :]
                g = grid[bases[0][:, None, None] + i, bases[1][None, :, None] + j, bases[2][None, None, :] + k]
                d += w[None] * np.moveaxis(g, -1, 0)
    return d


def coordinates(mat, out_shape, grid=None):
    """input index coordinates q [3, *out_shape] of every output voxel: q = M p + t + d(p)"""
    p = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in out_shape], indexing="ij"))
    M = np.asarray(mat, dtype=np.float64)
    q = np.einsum("ij,j...->i...", M[:, :3], p) + M[:, 3].reshape(3, 1, 1, 1)
    if grid is not None:
        q = q + displacement(np.asarray(grid, dtype=np.float64), out_shape)
    return q


def inside(q, in_shape):
    ok = np.ones(q.shape[1:], bool)
    for a in range(3):
        ok &= (q[a] >= -0.5) & (q[a] < in_shape[a] - 0.5)
    return ok


def sample(x, q, mode, pad=0.0):
    """x [C, *in_shape] at coordinates q: 'nearest', 'linear' or 'bspline' (x already holds the coefficients)"""
    in_shape = x.shape[1:]
    ok = inside(q, in_shape)
    C = x.shape[0]
    out = np.empty((C,) + q.shape[1:], dtype=np.float64 if mode != "nearest" else x.dtype)
    if mode == "nearest":
        idx = [np.clip(np.floor(q[a] + 0.5).astype(np.int64), 0, in_shape[a] - 1) for a in range(3)]
        for c in range(C):
            out[c] = x[c][tuple(idx)]
    elif mode == "linear":
        fl = [np.floor(q[a]) for a in range(3)]
        f = [q[a] - fl[a] for a in range(3)]
        i0 = [np.clip(fl[a].astype(np.int64), 0, in_shape[a] - 1) for a in range(3)]
        i1 = [np.clip(fl[a].astype(np.int64) + 1, 0, in_shape[a] - 1) for a in range(3)]
        for c in range(C):
            acc = 0.0
            for i in range(2):
                for j in range(2):
                    for k in range(2):
                        w = (f[0] if i else 1 - f[0]) * (f[1] if j else 1 - f[1]) * (f[2] if k else 1 - f[2])
                        acc = acc + w * x[c][(i1[0] if i else i0[0]), (i1[1] if j else i0[1]), (i1[2] if k else i0[2])]
            out[c] = acc
    else:
        fl = [np.floor(q[a]) for a in range(3)]
        w = [bspline_weights(q[a] - fl[a]) for a in range(3)]
        idx = [[mirror(fl[a].astype(np.int64) - 1 + k, in_shape[a]) for k in range(4)] for a in range(3)]
        for c in range(C):
            acc = 0.0
            for i in range(4):
                for j in range(4):
                    for k in range(4):
                        acc = acc + w[0][i] * w[1][j] * w[2][k] * x[c][idx[0][i], idx[1][j], idx[2][k]]
            out[c] = acc
    pad = np.broadcast_to(np.asarray(pad, dtype=np.float64).reshape(-1, 1, 1, 1) if np.ndim(pad) else pad,
                          (C, 1, 1, 1)) if mode != "nearest" else pad
    return np.where(ok[None], out, pad)


def otsu_pad(x, bins=128):
    """per channel: mean of the face voxels at or below the Otsu split of their `bins`-bin histogram (float32 binning)"""
    out = []
    for c in x:
        c = c.astype(np.float32)
        faces = np.hstack([f.ravel() for f in (c[0], c[-1], c[:, 0], c[:, -1], c[:, :, 0], c[:, :, -1])])
        mn, mx = faces.min(), faces.max()
        scale = np.float32(bins) / (mx - mn) if mx > mn else np.float32(0)
        b = np.minimum(((faces - mn) * scale).astype(np.int64), bins - 1)
        h = np.bincount(b, minlength=bins).astype(np.float64)
        centres = np.arange(bins) + 0.5
        tot, totm = h.sum(), (h * centres).sum()
        w0 = m0 = 0.0
        best, bv = bins - 1, -1.0
        for t in range(bins - 1):
            w0 += h[t]
            m0 += h[t] * centres[t]
            w1 = tot - w0
            if w0 == 0 or w1 == 0:
                continue
            d = m0 / w0 - (totm - m0) / w1
            v = w0 * w1 * d * d
            if v > bv:
                bv, best = v, t
        sel = faces[b <= best] if best < bins - 1 else faces
        out.append(sel.astype(np.float64).mean() if sel.size else faces.astype(np.float64).mean())
    return np.array(out)


# ------------------------------------------------------------------------------------------------ intensity
def bias_field(shape, coefficients, order=3):
    coords = [np.array([0.0]) if n == 1 else (2 * np.arange(n) - (n - 1)) / (n - 1) for n in shape]
    X, Y, Z = np.meshgrid(*coords, indexing="ij")
    acc = np.zeros(shape)
    i = 0
    for a in range(order + 1):
        for b in range(order + 1 - a):
            for c in range(order + 1 - a - b):
                acc += coefficients[i] * X ** a * Y ** b * Z ** c
                i += 1
    return np.exp(acc)


def percentile(x, q):
    return np.percentile(np.asarray(x, dtype=np.float64).ravel(), q)


def rescale(x, out_min_max, percentiles=(0, 100)):
    lo, hi = percentile(x, percentiles[0]), percentile(x, percentiles[1])
    if np.float32(lo) == np.float32(hi):
        return x
    y = np.clip(x, lo, hi)
    return (y - lo) / (hi - lo) * (out_min_max[1] - out_min_max[0]) + out_min_max[0]


def gamma(x, gammas):
    g = np.asarray(gammas, dtype=np.float64).reshape(-1, 1, 1, 1)
    return np.sign(x) * np.abs(x) ** g


def philox4x32(counter_lo, counter_hi, seed):
    """Philox4x32-10 of counters (lo, hi, 0, 0) under key = seed: the four uint32 output words"""
    c = [np.asarray(counter_lo, np.uint64) & _M32, np.asarray(counter_hi, np.uint64) & _M32,
         np.zeros_like(np.asarray(counter_lo, np.uint64)), np.zeros_like(np.asarray(counter_lo, np.uint64))]
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & _M32, p1 >> np.uint64(32), p1 & _M32
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
        k0 = (k0 + np.uint64(0x9E3779B9)) & _M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & _M32
    return c


def normal_stream(n, seed):
    i = np.arange(n, dtype=np.uint64)
    w = philox4x32(i & _M32, i >> np.uint64(32), seed)
    u1 = (w[0].astype(np.float64) + 1.0) * 2.0 ** -32
    u2 = w[1].astype(np.float64) * 2.0 ** -32
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def noise(x, mean, std, seed):
    return x + (mean + std * normal_stream(x.size, seed).reshape(x.shape))


def gaussian_blur(x, sigmas_vox):
    """scipy gaussian_filter(mode='reflect', truncate=4.0) per channel, restated with explicit reflected indices"""
    out = np.asarray(x, dtype=np.float64)
    for axis, s in enumerate(sigmas_vox):
        if s <= 0:
            continue
        r = int(4.0 * s + 0.5)
        w = np.exp(-0.5 / (s * s) * np.arange(-r, r + 1) ** 2)
        w /= w.sum()
        n = out.shape[axis + 1]
        idx = np.arange(n)[:, None] + np.arange(-r, r + 1)[None, :]
        idx = idx % (2 * n)
        idx = np.where(idx >= n, 2 * n - 1 - idx, idx)
        moved = np.moveaxis(out, axis + 1, -1)
        out = np.moveaxis((moved[..., idx] * w).sum(-1), -1, axis + 1)
    return out
