"""Numpy twin of the STEVE epoch visualisation (csrc/slot_vis.hip, focus_amd/slowfast/utils/slot_misc.py).

It restates, independently of both:
  * torchvision's make_grid for a 4-D batch (canvas of pad_value, image k at grid row k // xmaps, column k % xmaps, `padding`
    pixels between and around the images) and the reference's visualize loop (slot_misc.py:16-35: per frame one concatenate
    of video, recon_dvae, recon_tf and the K overlays, one make_grid with nrow = K + 3 and pad_value 0.8);
  * the overlay of steve.py:314-319: the slot update's attention [B,T,N,K] transposed to [B,T,K,1,He,We], repeated sy x sx
    (nearest upsampling), then video * a + (1 - a) as three fp32 operations, each rounded on its own (numpy never fuses);
  * TensorBoard's rule for a video (torch/utils/tensorboard/summary.py:video): (x * 255).clip(0, 255).astype(uint8) on
    fp32, i.e. truncation; a NaN is taken to 0 (numpy leaves that cast undefined; the kernel's header fixes it).

`mutant` names a deliberate mistake; the CPU tests check that each one changes the result on the inputs the tests use."""
import numpy as np

PAD = np.float32(0.8)
MUTANTS = ("fma", "swap_strides", "origin", "transposed", "round")


def grid_shape(T, H, W, K, rows):
    return (1, T, 3, rows * (H + 2) + 2, (K + 3) * (W + 2) + 2)


def make_grid(tiles, nrow, padding=2, pad_value=0.0, mutant=None):
    """tiles [N,C,H,W] float32 -> [C, ymaps (H + padding) + padding, xmaps (W + padding) + padding]."""
    n, c, h, w = tiles.shape
    xmaps = min(nrow, n)
    ymaps = -(-n // xmaps)
    height, width = h + padding, w + padding
    grid = np.full((c, height * ymaps + padding, width * xmaps + padding), pad_value, dtype=np.float32)
    off = 0 if mutant == "origin" else padding
    for k in range(n):
        y, x = divmod(k, xmaps)
        if mutant == "transposed":
            x, y = divmod(k, ymaps)
            if x >= xmaps:
                continue
        grid[:, y * height + off:y * height + off + h, x * width + off:x * width + off + w] = tiles[k]
    return grid


def visualize(video, recon_dvae, recon_tf, attns, num_slots, N=8, mutant=None):
    """All float32: video, recon_dvae [B,T,3,H,W], recon_tf [>= min(N,B),T,3,H,W], attns [B,T,K,3,H,W] -> [1,T,3,Hg,Wg]."""
    T = video.shape[1]
    frames = []
    for t in range(T):
        tiles = np.concatenate((video[:N, t, None], recon_dvae[:N, t, None], recon_tf[:N, t, None], attns[:N, t]), axis=1)
        tiles = tiles.reshape((-1,) + tiles.shape[2:])
        frames.append(make_grid(tiles, nrow=num_slots + 3, pad_value=PAD, mutant=mutant))
    return np.stack(frames, axis=0)[None]


def upsample(attn, grid, H, W, mutant=None):
    """attn [B,T,He*We,K] float32 -> masks [B,T,K,1,H,W]: cell (y // sy, x // sx) at pixel (y, x)."""
    He, We = grid
    B, T, N, K = attn.shape
    assert N == He * We and H % He == 0 and W % We == 0
    sy, sx = H // He, W // We
    m = attn.astype(np.float32).transpose(0, 1, 3, 2).reshape(B, T, K, 1, He, We)
    if mutant == "swap_strides":
        # the cell of pixel (y, x) taken as (y // sx, x // sy), clamped to the grid
        ys = np.minimum(np.arange(H) // sx, He - 1)
        xs = np.minimum(np.arange(W) // sy, We - 1)
        return m[..., ys, :][..., xs]
    return np.repeat(np.repeat(m, sy, axis=-2), sx, axis=-1)


def overlay(video, masks, mutant=None):
    """video [B,T,3,H,W], masks [B,T,K,1,H,W] -> video * a + (1 - a) [B,T,K,3,H,W], three fp32 roundings."""
    v = video.astype(np.float32)[:, :, None]
    a = masks.astype(np.float32)
    one_minus = (np.float32(1.0) - a).astype(np.float32)
    if mutant == "fma":
        # one rounding of v * a + (1 - a): the product of two fp32 numbers is exact in double
        return (v.astype(np.float64) * a.astype(np.float64) + one_minus.astype(np.float64)).astype(np.float32)
    prod = (v * a).astype(np.float32)
    return (prod + one_minus).astype(np.float32)


def visualize_slots(video, recon_dvae, recon_tf, attn, grid, N=8, mutant=None):
    """The raw form: the overlays are made from attn [B,T,He*We,K] and the video, then visualize()."""
    H, W = video.shape[-2:]
    vis = overlay(video, upsample(attn, grid, H, W, mutant), mutant)
    return visualize(video, recon_dvae, recon_tf, vis, attn.shape[3], N, mutant)


def to_uint8(x, mutant=None):
    with np.errstate(invalid="ignore"):
        y = (x.astype(np.float32) * np.float32(255.0)).astype(np.float32)
        y = np.where(np.isnan(y), np.float32(0.0), np.clip(y, np.float32(0.0), np.float32(255.0)))
        if mutant == "round":
            y = np.rint(y)
        return y.astype(np.uint8)


def bf16_round(x):
    """float32 -> the nearest bfloat16 (ties to even), returned as float32."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(np.float32)


def inputs(B, T, K, grid, H, W, seed, Bg=None):
    """Deterministic test inputs: video, recon, gen in [0,1), attn = a softmax over the K slots of every cell."""
    rng = np.random.default_rng(seed)
    Bg = B if Bg is None else Bg
    video = rng.random((B, T, 3, H, W), dtype=np.float32)
    recon = rng.random((B, T, 3, H, W), dtype=np.float32)
    gen = rng.random((Bg, T, 3, H, W), dtype=np.float32)
    logits = rng.standard_normal((B, T, grid[0] * grid[1], K)).astype(np.float32)
    e = np.exp(logits - logits.max(-1, keepdims=True))
    attn = (e / e.sum(-1, keepdims=True)).astype(np.float32)
    return video, recon, gen, attn
