"""Reference of the clip sampling kernel (focus_clip_sample, include/focus_amd.h): the single-pass formula in fp64, an fp32
twin of it, named wrong variants ("mutants") of it, and an error bound that is derived here, not tuned.

    xo = flip ? out_w-1-x : x
    sy = max((y  + oy0 + 0.5) * (sh / rh) - 0.5, 0);  y0 = min(int(sy), sh-1);  y1 = min(y0+1, sh-1);  ly = sy - y0
    sx = max((xo + ox0 + 0.5) * (sw / rw) - 0.5, 0);  x0, x1, lx likewise
    v  = bilinear of src[t][sy0 + y{0,1}][sx0 + x{0,1}][c'],  c' = reverse ? 2-c : c
    out[c][t][y][x] = (v/255 - mean[c']) / std[c']

The bound, per output element, against the fp64 result r (u = 2^-24, the unit roundoff of fp32):

  coordinate term  An fp32 implementation (ATen's as well as the kernel's) rounds the scale, the product and the
      subtraction that give sy and sx: three roundings of quantities no larger than the largest source coordinate + 1,
      so |d sy| <= 3 u (sh + 1) and |d sx| <= 3 u (sw + 1)  (ly = sy - y0 is then exact).  The bilinear interpolant is
      continuous and piecewise linear in sy and in sx with a slope of at most one full step between neighbouring pixel values,
      255 levels = 1 / min|std| in normalised units, so the value moves by at most (|d sy| + |d sx|) / min|std|.
  arithmetic term  N_ROUNDINGS fp32 roundings between the bytes and the result, each of relative size u on a quantity that,
      expressed in output units, is at most M = max_c max(1, |mean_c|, |1 - mean_c|) / |std_c|  (interpolation weights are
      convex, so a rounding in one tap or one row is not amplified).  Counted for the reference's order of operations, the
      longer of the two: /255, -mean, /std (3); 1-lx, 1-ly (2); two products and a sum along x (3); two products and a sum
      along y (3); one for the final store = 12.  The kernel's order (two lerps of exact byte differences, one fused
      multiply-add with two rounded constants) has fewer.
  bf16 output adds 2^-8 |r|.

A case with scale exactly 1 and whole-pixel offsets has sy, sx exact, and only the arithmetic term applies (coords=False)."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clip_sampling.npz")
U = 2.0 ** -24
N_ROUNDINGS = 12
MEAN, STD = [0.45, 0.40, 0.35], [0.225, 0.25, 0.2]          # distinct per channel: a wrong channel index shows

MUTANTS = ("align_corners", "no_max0", "no_tap_clamp", "flip_before_offset", "norm_by_output_channel", "inverse_scale")

# the fixture's cases: tag -> (clip, keyword arguments of spatial_sampling / sampling_params); the seeds are in the fixture
RATIO = [0.75, 1.3333]
CASES = {
    "rrc_noflip": ("a", dict(spatial_idx=-1, min_scale=22, max_scale=28, crop_size=13, scale=[0.08, 1.0], aspect_ratio=RATIO)),
    "rrc_flip": ("a", dict(spatial_idx=-1, min_scale=22, max_scale=28, crop_size=13, scale=[0.08, 1.0], aspect_ratio=RATIO)),
    "rrc_fallback": ("b", dict(spatial_idx=-1, min_scale=22, max_scale=28, crop_size=13, scale=[0.9, 1.0], aspect_ratio=RATIO)),
    "jitter": ("a", dict(spatial_idx=-1, min_scale=22, max_scale=28, crop_size=16)),
    "jitter_inv": ("b", dict(spatial_idx=-1, min_scale=18, max_scale=24, crop_size=16, inverse_uniform_sampling=True)),
    "test0": ("a", dict(spatial_idx=0, min_scale=16, max_scale=16, crop_size=16)),
    "test1": ("a", dict(spatial_idx=1, min_scale=16, max_scale=16, crop_size=16)),
    "test2": ("a", dict(spatial_idx=2, min_scale=16, max_scale=16, crop_size=16)),
}


def _axis(n_out, off, s_len, r_len, flip, f, mutant, lim):
    """Source taps and weight along one axis: (i0, i1, l), i relative to the rectangle.  lim: the last index that may be
    read when the second-tap clamp is missing (the mutant reads the neighbour outside the rectangle)."""
    o = np.arange(n_out)
    if flip and mutant == "flip_before_offset":
        pos = r_len - 1 - (o + off)                              # mirrors the whole resized image, then takes the window
    else:
        pos = (n_out - 1 - o if flip else o) + off
    if mutant == "align_corners":
        s = pos.astype(f) * (f(s_len - 1) / f(max(r_len - 1, 1)))
    else:
        scale = f(r_len) / f(s_len) if mutant == "inverse_scale" else f(s_len) / f(r_len)
        s = (pos.astype(f) + f(0.5)) * scale - f(0.5)
    if mutant != "no_max0":
        s = np.maximum(s, f(0))
    i0 = np.minimum(s.astype(np.int64), s_len - 1)
    i1 = np.minimum(i0 + 1, lim) if mutant == "no_tap_clamp" else np.minimum(i0 + 1, s_len - 1)
    return i0, i1, (s - i0.astype(f)).astype(f)


def sample(src, p, out_h, out_w, mean, std, reverse, dtype=np.float64, mutant=None):
    """src uint8 [T,H,W,3], p the descriptor fields -> [3,T,out_h,out_w] in `dtype` arithmetic (np.float64: the reference;
    np.float32: its twin)."""
    f = dtype
    T, H, W, _ = src.shape
    y0, y1, ly = _axis(out_h, p["oy0"], p["sh"], p["rh"], False, f, mutant, H - 1 - p["sy0"])
    x0, x1, lx = _axis(out_w, p["ox0"], p["sw"], p["rw"], bool(p["flip"]), f, mutant, W - 1 - p["sx0"])
    y0, y1, x0, x1 = y0 + p["sy0"], y1 + p["sy0"], x0 + p["sx0"], x1 + p["sx0"]
    s = src.astype(f)
    ly, lx = ly[None, :, None, None], lx[None, None, :, None]
    one = f(1)
    top = (one - lx) * s[:, y0][:, :, x0] + lx * s[:, y0][:, :, x1]
    bot = (one - lx) * s[:, y1][:, :, x0] + lx * s[:, y1][:, :, x1]
    v = (one - ly) * top + ly * bot                              # [T, out_h, out_w, 3 source channels]
    out = np.empty((3, T, out_h, out_w), dtype=f)
    for c in range(3):
        cs = 2 - c if reverse else c
        cn = c if mutant == "norm_by_output_channel" else cs
        out[c] = (v[..., cs] / f(255) - f(mean[cn])) / f(std[cn])
    return out


def bound(p, mean, std, ref=None, bf16=False, coords=True):
    """Admissible |result - fp64 reference| (scalar, or per element with bf16), see the module docstring."""
    inv_std = 1.0 / min(abs(float(s)) for s in std)
    m = max(max(1.0, abs(float(a)), abs(1.0 - float(a))) / abs(float(s)) for a, s in zip(mean, std))
    tol = N_ROUNDINGS * U * m
    if coords:
        tol += 3 * U * ((p["sh"] + 1) + (p["sw"] + 1)) * inv_std
    if bf16:
        tol = tol + 2.0 ** -8 * np.abs(ref)
    return tol


def ratio(got, ref, tol):
    """max |got - ref| / tol: inside the bound iff <= 1."""
    return float(np.max(np.abs(np.asarray(got, dtype=np.float64) - ref) / tol))


def fixture():
    return np.load(GOLDEN, allow_pickle=False)
